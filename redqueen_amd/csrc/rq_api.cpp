// rq_api.cpp -- the HIP side of the C ABI declared in include/rq.h.
//
// The host arithmetic lives in the HIP-free host core (rq_host.h): rq_topo.cpp builds the
// graph topology and the controller tables, rq_plan.cpp plans a batch and reads the
// environment knobs.  Here: rq_graph_build uploads the topology once, rq_run_batch stages
// the per-run tables and enqueues the kernels of every chunk, and thin wrappers launch the
// replay, analysis and log kernels.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <mutex>
#include <new>
#include <vector>

#include "../../include/rq.h"
#include "rq_internal.h"

using rqh::align_up;
using rqh::CtrlTables;
using rqh::GraphTopo;
using rqh::Knobs;
using rqh::Plan;

namespace {

template <class T>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
    ~DevBuf() { if (p) (void)hipFree(p); }
    int upload(const std::vector<T>& v)
    {
        n = v.size();
        if (hipMalloc(&p, std::max<size_t>(1, n) * sizeof(T)) != hipSuccess) return RQ_ENOMEM;
        if (n && hipMemcpy(p, v.data(), n * sizeof(T), hipMemcpyHostToDevice) != hipSuccess)
            return RQ_EHIP;
        return RQ_OK;
    }
};

// Optional per-kernel timing (rq_timing): HIP events recorded on the launch
// stream around every kernel, summed by rq_timing_read.  Off by default.
enum { K_GEN = 0, K_SWEEP = 1, K_SCAN = 2, K_REPLAY = 3, K_MERGE = 4, K_N = 5 };
bool g_timing = false;
unsigned long long* g_clk = nullptr;   // RQ_PHASE_CLOCK builds: the sweep's / merge's phase clocks
#ifdef RQ_PHASE_CLOCK
unsigned long long* phase_clk()
{
    if (!g_clk && hipMalloc(&g_clk, 8 * sizeof(unsigned long long)) == hipSuccess)
        (void)hipMemset(g_clk, 0, 8 * sizeof(unsigned long long));
    return g_clk;
}
#endif

std::vector<std::pair<hipEvent_t, hipEvent_t>> g_ev[K_N];

struct TimedLaunch {
    int k;
    hipStream_t s;
    hipEvent_t a = nullptr, b = nullptr;
    TimedLaunch(int k_, hipStream_t s_) : k(k_), s(s_)
    {
        if (g_timing && hipEventCreate(&a) == hipSuccess && hipEventCreate(&b) == hipSuccess)
            (void)hipEventRecord(a, s);
    }
    ~TimedLaunch()
    {
        if (a && b) {
            (void)hipEventRecord(b, s);
            g_ev[k].push_back({a, b});
        }
    }
};

// Side streams of the pipelined chunk loop (rq_run_batch): per host thread AND per
// caller stream, created on first use on the caller's current device, with the fork /
// join events.  Work on them is always bracketed by a wait on the caller's stream (fork)
// and a wait of the caller's stream on them (join), so the call stays stream-ordered for
// the caller; batches issued on different caller streams get different side streams and
// so overlap (a caller alternating two streams overlaps one batch's tail with the next
// batch's generation and merge).
struct SidePipe {
    int dev = -1;
    hipStream_t caller = nullptr;
    uint64_t used = 0;   // last use (SidePipes' LRU clock)
    hipStream_t s[2] = {nullptr, nullptr};
    hipEvent_t fork = nullptr, join[2] = {nullptr, nullptr};
    // drop the streams and events (made on device `dev`) once their work is done
    void release()
    {
        if (dev < 0) return;
        int cur = -1;
        (void)hipGetDevice(&cur);
        if (cur != dev) (void)hipSetDevice(dev);
        for (int k = 0; k < 2; ++k) {
            if (s[k]) {
                (void)hipStreamSynchronize(s[k]);
                (void)hipStreamDestroy(s[k]);
            }
            if (join[k]) (void)hipEventDestroy(join[k]);
            s[k] = nullptr;
            join[k] = nullptr;
        }
        if (fork) (void)hipEventDestroy(fork);
        fork = nullptr;
        if (cur >= 0 && cur != dev) (void)hipSetDevice(cur);
        dev = -1;
    }
    int get(int n, hipStream_t* out)
    {
        int d = 0;
        if (hipGetDevice(&d) != hipSuccess) return RQ_EHIP;
        if (dev != d) {   // first use (or another device's pipe re-homed): fresh streams and events
            release();
            dev = d;
        }
        if (!fork && hipEventCreateWithFlags(&fork, hipEventDisableTiming) != hipSuccess) return RQ_EHIP;
        for (int k = 0; k < n && k < 2; ++k) {
            if (!s[k] && hipStreamCreateWithFlags(&s[k], hipStreamNonBlocking) != hipSuccess) return RQ_EHIP;
            if (!join[k] && hipEventCreateWithFlags(&join[k], hipEventDisableTiming) != hipSuccess) return RQ_EHIP;
            out[k] = s[k];
        }
        return RQ_OK;
    }
};
// a few (device, caller stream) pairs per thread (the engine's users run on one or two
// streams); the null stream has the same handle on every device, hence the device in the
// key.  Past kPipes the least recently used entry is re-homed: on the same device its
// streams and events are kept (only the owner changes), on another they are destroyed
// once idle and made afresh.
constexpr int kPipes = 4;
struct SidePipes {
    SidePipe p[kPipes];
    uint64_t clock = 0;
    SidePipe& of(hipStream_t caller)
    {
        int d = -1;
        (void)hipGetDevice(&d);
        SidePipe* lru = &p[0];
        for (SidePipe& x : p) {
            if (x.used && x.caller == caller && (x.dev == d || x.dev < 0)) {
                x.used = ++clock;
                return x;
            }
            if (x.used < lru->used) lru = &x;
        }
        if (lru->dev >= 0 && lru->dev != d) lru->release();
        lru->caller = caller;
        lru->used = ++clock;
        return *lru;
    }
    // no destructor: a thread's pipes live until the process ends (HIP may already be
    // torn down when thread_local destructors run at exit)
};
thread_local SidePipes t_pipes;

}  // namespace

namespace {
constexpr int kStages = 4;
struct Stage {
    void* buf = nullptr;
    size_t bytes = 0;
    hipEvent_t done = nullptr;
};
}  // namespace

// the topology (rq_host.h), its device copies and the staging ring
struct rq_graph : GraphTopo {
    DevBuf<int64_t> d_sink_ids, d_src_id;
    DevBuf<int> d_csr_col_el, d_lay_ptr, d_lay_end;
    DevBuf<int> d_tile_ptr, d_tile_col;   // the sink-tiled CSR (n_tiles > 0)
    DevBuf<uint32_t> d_mask, d_fbits;
    DevBuf<int> d_kind, d_orig, d_arr_off, d_arr_n, d_csr_ptr, d_csr_col, d_outdeg_f, d_fol, d_cbf, d_gen_cls;
    DevBuf<uint32_t> d_seed;
    DevBuf<double> d_p0, d_p1, d_p2, d_arr_a, d_arr_b;
    int upload();
    // pinned staging ring for the per-run parameter tables
    std::mutex stage_mu;
    Stage stage[kStages];
    int stage_next = 0;
    ~rq_graph()
    {
        for (Stage& st : stage) {
            if (st.done) {
                (void)hipEventSynchronize(st.done);
                (void)hipEventDestroy(st.done);
            }
            if (st.buf) (void)hipHostFree(st.buf);
        }
    }
};

int rq_graph::upload()
{
    int rc;
    if (nw > 0 && (rc = d_mask.upload(masks))) return rc;
    if ((rc = d_fbits.upload(fbits))) return rc;
    if ((rc = d_src_id.upload(src_id)) || (rc = d_kind.upload(kind)) ||
        (rc = d_orig.upload(orig_idx)) || (rc = d_arr_off.upload(arr_off)) ||
        (rc = d_arr_n.upload(arr_n)) || (rc = d_csr_ptr.upload(csr_ptr)) ||
        (rc = d_csr_col.upload(csr_col)) || (rc = d_outdeg_f.upload(outdeg_f)) ||
        (rc = d_fol.upload(fol)) || (rc = d_seed.upload(seed)) ||
        (rc = d_p0.upload(p0)) || (rc = d_p1.upload(p1)) ||
        (rc = d_p2.upload(p2)) || (rc = d_arr_a.upload(arr_a)) ||
        (rc = d_arr_b.upload(arr_b)) || (rc = d_sink_ids.upload(sink_ids)) ||
        (rc = d_csr_col_el.upload(csr_col_el)) || (rc = d_cbf.upload(cbf)) ||
        (rc = d_gen_cls.upload(gen_cls)))
        return rc;
    if (multi && ((rc = d_lay_ptr.upload(lay_ptr)) || (rc = d_lay_end.upload(lay_end))))
        return rc;
    if (n_tiles > 0 && ((rc = d_tile_ptr.upload(tile_ptr)) || (rc = d_tile_col.upload(tile_col))))
        return rc;
    return RQ_OK;
}

namespace {

// device-memory budget of a plan's workspace: the caller's (rq_batch_desc.ws_budget),
// else `fallback` (rq_run_batch: the workspace it was handed) or, with none, 0.9 x the
// device's free memory; RQ_WS_BUDGET_GB caps it
double ws_budget(const rq_batch_desc* b, const Knobs& kn, double fallback)
{
    double bud = b && b->ws_budget > 0 ? (double)b->ws_budget : fallback;
    if (!(bud > 0.0)) {
        size_t fr = 0, tot = 0;
        bud = hipMemGetInfo(&fr, &tot) == hipSuccess ? 0.9 * (double)fr : 200.0 * (1 << 30);
    }
    if (kn.ws_budget_gb.set) bud = std::min(bud, kn.ws_budget_gb.v * (1 << 30));
    return bud;
}

// the plan of an ABI call, under the knobs the call read at its start
int plan_call(const rq_graph* g, const rq_batch_desc* b, const Knobs& kn, double fallback, Plan* p)
{
    if (!g || !b) return RQ_EINVAL;
    return rqh::make_plan(*g, b, kn, ws_budget(b, kn, fallback), p);
}

// ---- rq_run_batch in parts ----

// Parameter tables [inv_c | st_off | cap | rd_k | rep_idx | pw_c | pw_max] to the start of
// the workspace: staged in one of the graph's pinned host buffers so the copy is truly
// asynchronous (a pageable copy would stall the host)
// The next slot of the graph's pinned ring, at least `bytes` large and free again (the copy
// issued from it four calls ago is done).  The caller holds stage_mu, fills slot->buf, copies
// from it on its stream and records slot->done there.
int stage_slot(rq_graph* g, size_t bytes, Stage** slot)
{
    Stage& st = g->stage[g->stage_next];
    g->stage_next = (g->stage_next + 1) % kStages;
    if (st.bytes < bytes) {
        // grow the whole ring at once (pinned allocation is slow: never leave a stage
        // to be allocated by a later, possibly timed, call); round up to 64 KiB
        const size_t want = align_up(bytes, (size_t)65536);
        for (Stage& x : g->stage) {
            if (x.done && hipEventSynchronize(x.done) != hipSuccess) return RQ_EHIP;
            if (x.bytes >= want) continue;
            if (x.buf) (void)hipHostFree(x.buf);
            x.buf = nullptr;
            x.bytes = 0;
            if (hipHostMalloc(&x.buf, want, hipHostMallocDefault) != hipSuccess) return RQ_ENOMEM;
            x.bytes = want;
            if (!x.done && hipEventCreateWithFlags(&x.done, hipEventDisableTiming) != hipSuccess)
                return RQ_EHIP;
        }
    }
    if (st.done && hipEventSynchronize(st.done) != hipSuccess) return RQ_EHIP;
    *slot = &st;
    return RQ_OK;
}

int stage_tables(rq_graph* g, const Plan& p, const rq_batch_desc* b, const CtrlTables& t, char* ws,
                 hipStream_t s)
{
    std::lock_guard<std::mutex> lk(g->stage_mu);
    Stage* slot = nullptr;
    const int rc = stage_slot(g, p.tables_bytes, &slot);
    if (rc != RQ_OK) return rc;
    Stage& st = *slot;
    char* tab = (char*)st.buf;
    std::memcpy(tab + p.off_invc, t.invc.data(), t.invc.size() * sizeof(double));
    std::memcpy(tab + p.off_stoff, p.st_off.data(), p.st_off.size() * sizeof(int64_t));
    std::memcpy(tab + p.off_cap, p.cap.data(), p.cap.size() * sizeof(int));
    std::memcpy(tab + p.off_rdk, p.rd_k.data(), p.rd_k.size() * sizeof(int));
    if (b->rep_idx) std::memcpy(tab + p.off_repidx, b->rep_idx, sizeof(int64_t) * (size_t)p.R);
    if (!t.pwc.empty()) {
        std::memcpy(tab + p.off_pwc, t.pwc.data(), t.pwc.size() * sizeof(double));
        std::memcpy(tab + p.off_pwmax, t.pwmax.data(), t.pwmax.size() * sizeof(double));
    }
    if (hipMemcpyAsync(ws, tab, p.tables_bytes, hipMemcpyHostToDevice, s) != hipSuccess ||
        hipEventRecord(st.done, s) != hipSuccess)
        return RQ_EHIP;
    return RQ_OK;
}

// The join of the side streams on EVERY exit: an error return inside the chunk loop
// must not leave work queued on a side stream that writes the caller's buffers after
// the caller's stream has moved on (the caller frees them when the call fails)
struct Join {
    hipStream_t* pst;
    SidePipe& sp;
    int n = 1;
    int done()
    {
        int rc = RQ_OK;
        for (int k = 1; k < n; ++k)
            if (hipEventRecord(sp.join[k - 1], pst[k]) != hipSuccess ||
                hipStreamWaitEvent(pst[0], sp.join[k - 1], 0) != hipSuccess)
                rc = RQ_EHIP;
        n = 1;
        return rc;
    }
    ~Join() { (void)done(); }
};
// the fork: side streams pst[1 .. nbuf) wait for what the caller's stream pst[0] holds so
// far (the tables, the status memset); join->n counts the streams to join
int fork_streams(int nbuf, Join* join)
{
    if (nbuf <= 1) return RQ_OK;
    if (const int rc = join->sp.get(nbuf - 1, join->pst + 1)) return rc;
    if (hipEventRecord(join->sp.fork, join->pst[0]) != hipSuccess) return RQ_EHIP;
    for (int k = 1; k < nbuf; ++k) {
        if (hipStreamWaitEvent(join->pst[k], join->sp.fork, 0) != hipSuccess) return RQ_EHIP;
        join->n = k + 1;
    }
    return RQ_OK;
}

// one pass of the chunk loop: replicas [c0, c0 + C) of the call
struct Chunk {
    int64_t c0, C;
    char* ws;    // the workspace (the parameter tables at its start)
    char* wsb;   // this chunk's buffer set
};

GenArgs gen_args(const rq_graph* g, const Plan& p, const rq_batch_desc* b, const rq_outputs* out,
                 const Chunk& ch, const Knobs& kn)
{
    GenArgs ga{};
    ga.n_chunk = ch.C;
    ga.chunk0 = ch.c0;
    ga.rep0 = b->replica0;
    ga.n_rep = b->n_rep;
    ga.rep_lo = p.rep_lo;
    ga.rep_cnt = p.rep_cnt;
    ga.rep_idx = b->rep_idx ? (const int64_t*)(ch.ws + p.off_repidx) : nullptr;
    ga.n_str = g->n_str;
    ga.ctrl_idx = g->ctrl_idx;
    ga.ctrl_stream_kind =
        (b->ctrl_kind == RQ_SRC_OPT || b->ctrl_kind == RQ_SRC_OPTPW || b->ctrl_kind == RQ_SRC_NONE)
            ? RQ_SRC_NONE : b->ctrl_kind;
    ga.randomize = b->randomize_world;
    ga.seed_mod = b->seed_mod;
    ga.ctrl_seed = b->ctrl_seed;
    ga.ctrl_seed0 = b->ctrl_seed0;
    ga.world_seed = b->world_seed;
    ga.world_seed0 = b->world_seed0;
    ga.ctrl_rate = b->ctrl_rate;
    ga.kind = g->d_kind.p;
    ga.orig_idx = g->d_orig.p;
    ga.seed = g->d_seed.p;
    ga.p0 = g->d_p0.p;
    ga.p1 = g->d_p1.p;
    ga.p2 = g->d_p2.p;
    ga.arr_off = g->d_arr_off.p;
    ga.arr_n = g->d_arr_n.p;
    ga.arr_a = g->d_arr_a.p;
    ga.arr_b = g->d_arr_b.p;
    ga.st_off = (const int64_t*)(ch.ws + p.off_stoff);
    ga.cap = (const int*)(ch.ws + p.off_cap);
    ga.capsum = p.capsum;
    ga.start = g->start;
    ga.end = g->end;
    ga.streams = (double*)(ch.wsb + p.off_streams);
    ga.slen = (int*)(ch.wsb + p.off_slen);
    ga.slen_stride = p.chunk;
    ga.status = out->status;
    if (b->n_rd > 0) {
        ga.rd_k = (const int*)(ch.ws + p.off_rdk);
        ga.n_rd = b->n_rd;
        ga.rd_times = b->rd_times;
        ga.rd_off = b->rd_off;
    }
    if (kn.gen_split) {
        ga.cls = g->d_gen_cls.p;
        for (int c = 0; c < 3; ++c) ga.cls_n[c] = g->gen_n[c];
    }
    return ga;
}

// the one-level merge's arguments, which are the second level's of a two-level merge
// (launch_merge adds the groups)
MergeArgs merge_args(const rq_graph* g, const Plan& p, const rq_outputs* out, const Chunk& ch,
                     const GenArgs& ga, const Knobs& kn)
{
    MergeArgs ma{};
    ma.n_chunk = ch.C;
    ma.chunk0 = ch.c0;
    ma.n_str = g->n_str;
    ma.capsum = p.capsum;
    ma.st_off = ga.st_off;
    ma.streams = ga.streams;
    ma.slen = ga.slen;
    ma.slen_stride = ga.slen_stride;
    ma.end = g->end;
    ma.out_t = (double*)(ch.wsb + p.off_mt);
    ma.out_j = (uint16_t*)(ch.wsb + p.off_mj);
    ma.out_jh = g->n_str > 65535 ? (uint8_t*)(ch.wsb + p.off_mjh) : nullptr;
    ma.out_len = (int*)(ch.wsb + p.off_mlen);
    ma.mrg_stride = p.mrg_stride;
    ma.status = out->status;
    ma.strict_ties = p.lmrg ? 1 : 0;
#ifdef RQ_PHASE_CLOCK
    if (kn.clk_merge) ma.clk = phase_clk();   // else the sweep's phases only
#else
    (void)kn;
#endif
    return ma;
}

// rq_merge_streams for the chunk: one level, or (> RQ_MG_B sources) the groups, then the
// groups' sequences
int launch_merge(const Plan& p, MergeArgs ma, const Chunk& ch, hipStream_t s)
{
    TimedLaunch tl(K_MERGE, s);
    if (p.n_grp <= 1) return rq_launch_merge(ma, s) == hipSuccess ? RQ_OK : RQ_EHIP;
    // level 1: each group of grp_sz streams into its own sequence
    ma.grp_sz = p.grp_sz;
    MergeArgs m1 = ma;
    m1.out_t = (double*)(ch.wsb + p.off_sub_t);
    m1.out_j = (uint16_t*)(ch.wsb + p.off_sub_j);   // group-local streams: u16 always
    m1.out_jh = nullptr;
    m1.out_len = (int*)(ch.wsb + p.off_sub_len);
    m1.mrg_stride = p.sub_stride;
    if (rq_launch_merge_groups(m1, s) != hipSuccess) return RQ_EHIP;
    // level 2: the groups' sequences into the replica's play order
    ma.sub_t = m1.out_t;
    ma.sub_j = m1.out_j;
    ma.sub_len = m1.out_len;
    ma.n_grp = p.n_grp;
    ma.sub_stride = p.sub_stride;
    return rq_launch_merge_sub(ma, s) == hipSuccess ? RQ_OK : RQ_EHIP;
}

SweepArgs sweep_args(const rq_graph* g, const Plan& p, const rq_batch_desc* b, const rq_outputs* out,
                     const Chunk& ch, const GenArgs& ga, const Knobs& kn)
{
    char* ws = ch.ws;
    char* wsb = ch.wsb;
    SweepArgs sa{};
    sa.n_chunk = ch.C;
    sa.chunk0 = ch.c0;
    sa.n_rep = b->n_rep;
    sa.rep0 = b->replica0;
    sa.n_str = g->n_str;
    sa.n_sinks = g->n_sinks;
    sa.n_sinks_pad = p.n_sinks_pad;
    sa.ctrl_idx = g->ctrl_idx;
    sa.ctrl_kind = b->ctrl_kind;
    sa.n_fol = b->ctrl_kind == RQ_SRC_NONE ? 0 : g->n_fol;
    for (int q = 0; q < RQ_MAX_K; ++q) sa.Ks[q] = q < b->nK ? b->Ks[q] : 1;
    sa.ctrl_src_id = g->ctrl_src_id;
    sa.seed_mod = b->seed_mod;
    sa.ctrl_seed = b->ctrl_seed;
    sa.ctrl_seed0 = b->ctrl_seed0;
    sa.src_id = g->d_src_id.p;
    sa.inv_c = (const double*)(ws + p.off_invc);
    if (b->ctrl_kind == RQ_SRC_OPTPW) {
        sa.pw_c = (const double*)(ws + p.off_pwc);
        sa.pw_max = (const double*)(ws + p.off_pwmax);
        sa.n_seg = b->n_seg;
        sa.period = b->period;
    }
    sa.csr_ptr = g->d_csr_ptr.p;
    sa.csr_col = g->d_csr_col.p;
    sa.outdeg_f = g->d_outdeg_f.p;
    sa.cbf_g = g->d_cbf.p;
    sa.fol = g->d_fol.p;
    sa.st_off = (const int64_t*)(ws + p.off_stoff);
    sa.capsum = p.capsum;
    sa.streams = (const double*)(wsb + p.off_streams);
    sa.slen = (const int*)(wsb + p.off_slen);
    sa.slen_stride = p.chunk;
    if (p.mrg) {
        sa.mrg_t = (const double*)(wsb + p.off_mt);
        sa.mrg_j = (const uint16_t*)(wsb + p.off_mj);
        sa.mrg_jh = g->n_str > 65535 ? (const uint8_t*)(wsb + p.off_mjh) : nullptr;
        sa.mrg_len = (const int*)(wsb + p.off_mlen);
        sa.mrg_stride = p.mrg_stride;
        if (p.order) sa.order = (const int*)(wsb + p.off_ord);   // written by rq_launch_order
    }
    sa.start = g->start;
    sa.end = g->end;
    sa.max_events = b->max_events;
    sa.cap_rows = p.cap_rows;
    sa.rows_t = (double*)(wsb + p.off_rt);
    sa.rows_sum = (double*)(wsb + p.off_rs);
    sa.rows_valid = (uint32_t*)(wsb + p.off_rv);
    sa.rows_cnt = (uint32_t*)(wsb + p.off_rc);
    sa.sall = (int*)(wsb + p.off_sall);
    sa.counts = out->counts;
    sa.status = out->status;
    if (b->flags & RQ_RUN_EVENT_LOG) {
        sa.ev_t = out->ev_t;
        sa.ev_src = out->ev_src;
        sa.ev_cap = out->ev_cap;
    }
    sa.n_csr = (int)g->csr_col.size();
    sa.wpb = p.gwpb;
    sa.win = p.gwin;
    sa.col_in_lds = p.gcol_lds;
    sa.lds_col = p.g_col;
    sa.lds_ptr = p.g_ptr;
    sa.lds_odf = p.g_odf;
    sa.lds_cbf = p.g_cbf;
    sa.lds_wave = p.g_wave;
    sa.lds_wave_stride = p.g_wave_stride;
    sa.lds_rank_off = p.g_rank_off;
    sa.lds_win_off = p.g_win_off;
    sa.lds_x_off = p.g_x_off;
    sa.lay_ptr = g->multi ? g->d_lay_ptr.p : nullptr;
    sa.lay_end = g->multi ? g->d_lay_end.p : nullptr;
    if (p.gs) {
        sa.gs = ws + p.off_gs;
        sa.gs_stride = p.gs_stride;
        sa.gs_slots = (int)p.gs_slots;
    }
    sa.lds_mask = p.g_col;   // BITS: the bitsets take the columns' place
    sa.masks = g->d_mask.p;
    sa.nw = g->nw;
    sa.mstride = p.mstride;
    sa.fbits = g->d_fbits.p;
    sa.nwl = (g->n_sinks + 31) / 32;
    sa.lds_fbits = p.g_fb;
    sa.lds_skip = p.g_skip;
    sa.lds_etab = p.g_etab;
    sa.lds_invc = p.g_inv;
    sa.invc_shared = !p.fw && p.g_inv_sh;
    sa.dbg = kn.sweep_dbg;   // profiling only
    sa.tile_target = kn.fw_tile;
    // refill policy (C3, sweep ms): forced passes only when a ring shows < 2 arrivals
    // (the cut is bounded by each ring's last visible arrival), opportunistic passes
    // while >= n_str / 2 rings are below W -- (H, n/3) 4.12, (2, n/3) 3.86,
    // (2, n/2) 3.79, (2, 0.64 n) 3.89, (1, n/2) 3.84-3.88
    sa.fw_hmin = std::min(2, p.fw_h);
    if (kn.fw_hmin.set) sa.fw_hmin = std::max(1, std::min(p.fw_h, kn.fw_hmin.v));   // tuning only
    sa.fw_thr = g->n_str >= 6 ? (g->n_str + 1) / 2 : 2;
    if (kn.fw_thr.set) sa.fw_thr = std::max(1, kn.fw_thr.v);   // tuning only
    // a forced run (some ring < fw_hmin) ends once every ring shows H arrivals, not W:
    // (C3 sweep ms) fill to 16 3.85, 12 3.78, 8 3.69-3.71, 6 3.69, 4 3.71
    sa.fw_hfill = p.fw_h;
    if (kn.fw_hfill.set) sa.fw_hfill = std::max(1, std::min(p.gwin, kn.fw_hfill.v));   // tuning only
#ifdef RQ_PHASE_CLOCK
    if (!kn.clk_merge) sa.clk = phase_clk();   // RQ_CLK_MERGE: the eight sums are the merge's alone
#endif
    sa.lds_total = p.g_total;
    sa.metrics = out->metrics;
    sa.lds_stage_off = p.g_stage_off;
    sa.gen = ga;
    // waves past their first replica take the next one from a queue, so the launch tail is
    // spread over every CU instead of whole 16-wave blocks: both sweep kinds, unless
    // RQ_FW_STATIC (A/B only; GS needs the queue)
    if (!kn.fw_static || p.gs) sa.wq = (int*)(wsb + p.off_wq);
    return sa;
}

ScanArgs scan_args(const rq_graph* g, const Plan& p, const rq_outputs* out, const Chunk& ch,
                   const SweepArgs& sa)
{
    ScanArgs sc{};
    sc.n_chunk = ch.C;
    sc.chunk0 = ch.c0;
    sc.nrows = out->counts + 3;
    sc.nrows_stride = 4;
    sc.sall = (const int*)(ch.wsb + p.off_sall);
    sc.row_stride = p.cap_rows;
    sc.rows_t = sa.rows_t;
    sc.rows_sum = sa.rows_sum;
    sc.rows_valid = sa.rows_valid;
    sc.rows_cnt = sa.rows_cnt;
    sc.end = g->end;
    sc.metrics = out->metrics;
    sc.wq = (int*)(ch.wsb + p.off_wq) + 1;
    return sc;
}

}  // namespace

extern "C" {

int rq_abi_version(void) { return RQ_ABI_VERSION; }

const char* rq_strerror(int code)
{
    switch (code) {
    case RQ_OK: return "ok";
    case RQ_EINVAL: return "invalid argument";
    case RQ_EOVERFLOW: return "capacity overflow";
    case RQ_EHIP: return "HIP runtime error";
    case RQ_ENOMEM: return "out of memory";
    case RQ_EUNSORTED: return "dataframe t column is not sorted";
    case RQ_EUNSUPPORTED: return "unsupported by this engine";
    default: return "unknown error";
    }
}

int rq_graph_build(const rq_graph_desc* d, rq_graph_t* out)
{
    if (!d || !out) return RQ_EINVAL;
    *out = nullptr;
    std::unique_ptr<rq_graph> g(new (std::nothrow) rq_graph());
    if (!g) return RQ_ENOMEM;
    if (const int rc = rqh::topo_build(d, g.get())) return rc;
    if (const int rc = g->upload()) return rc;
    *out = g.release();
    return RQ_OK;
}

int rq_graph_free(rq_graph_t g)
{
    delete g;
    return RQ_OK;
}

int rq_graph_info(rq_graph_t g, int64_t* info)
{
    if (!g || !info) return RQ_EINVAL;
    info[0] = g->n_str;
    info[1] = g->n_sinks;
    info[2] = g->n_fol;
    info[3] = g->n_edges;
    info[4] = g->ctrl_idx;
    return RQ_OK;
}

int rq_graph_source_ids(rq_graph_t g, int64_t* ids)
{
    if (!g || !ids) return RQ_EINVAL;
    std::copy(g->src_id.begin(), g->src_id.end(), ids);
    return RQ_OK;
}

int rq_graph_followers(rq_graph_t g, int64_t* ids)
{
    if (!g || !ids) return RQ_EINVAL;
    std::copy(g->fol_ids.begin(), g->fol_ids.end(), ids);
    return RQ_OK;
}

int rq_workspace_size(rq_graph_t g, const rq_batch_desc* b, size_t* bytes)
{
    if (!bytes) return RQ_EINVAL;
    Plan p;
    const int rc = plan_call(g, b, rqh::read_knobs(), 0.0, &p);
    if (rc) return rc;
    *bytes = p.total;
    return RQ_OK;
}

int rq_plan_info(rq_graph_t g, const rq_batch_desc* b, int64_t* info)
{
    return rq_plan_info_n(g, b, info, 8);
}

int rq_plan_info_n(rq_graph_t g, const rq_batch_desc* b, int64_t* out, int n)
{
    if (!out || n < 0) return RQ_EINVAL;
    int64_t info[11];
    Plan p;
    const int rc = plan_call(g, b, rqh::read_knobs(), 0.0, &p);
    if (rc) return rc;
    rqh::plan_info(p, b->ctrl_kind, info);
    info[9] = p.blk ? 1 : 0;
    info[10] = p.rows16 ? 1 : 0;
    std::copy(info, info + std::min(n, 11), out);
    return RQ_OK;
}

int rq_event_capacity(rq_graph_t g, const rq_batch_desc* b, int64_t* cap)
{
    if (!cap) return RQ_EINVAL;
    Plan p;
    const int rc = plan_call(g, b, rqh::read_knobs(), 0.0, &p);
    if (rc) return rc;
    *cap = p.cap_rows;
    return RQ_OK;
}

int rq_run_batch(rq_graph_t g, const rq_batch_desc* b, const rq_outputs* out, void* workspace,
                 size_t workspace_bytes, void* hip_stream)
{
    const Knobs kn = rqh::read_knobs();
    Plan p;
    // the same plan as rq_workspace_size gave when the caller fixes the budget; else the
    // chunks that fit the workspace handed over
    int rc = plan_call(g, b, kn, (double)workspace_bytes, &p);
    if (rc) return rc;
    if (!out || !out->metrics || !out->counts || !out->status || !workspace) return RQ_EINVAL;
    if (workspace_bytes < p.total) return RQ_EINVAL;
    if ((b->flags & RQ_RUN_EVENT_LOG) && (!out->ev_t || !out->ev_src || out->ev_cap < 1))
        return RQ_EINVAL;
    char* ws = (char*)workspace;
    // pipelined chunks: chunk k runs on stream k % nbuf (the caller's stream and up to two
    // side streams, forked after the tables / status below and joined before returning)
    // with buffer set k % nbuf, so a set is reused only in its own stream's order
    hipStream_t pst[3] = {(hipStream_t)hip_stream, nullptr, nullptr};

    if ((rc = stage_tables(g, p, b, rqh::ctrl_tables(*g, b), ws, pst[0]))) return rc;
    if (hipMemsetAsync(out->status, 0, sizeof(int32_t) * p.R, pst[0]) != hipSuccess) return RQ_EHIP;
    Join join{pst, t_pipes.of(pst[0])};
    if ((rc = fork_streams(p.nbuf, &join))) return rc;

    int64_t ci = 0;
    for (int64_t c0 = 0; c0 < p.R; c0 += p.chunk, ++ci) {
        hipStream_t s = pst[ci % p.nbuf];
        const Chunk ch{c0, std::min(p.chunk, p.R - c0), ws,
                       ws + p.off_set0 + (size_t)(ci % p.nbuf) * p.set_stride};
        // gen (the generating fused sweep makes its arrivals itself)
        const GenArgs ga = gen_args(g, p, b, out, ch, kn);
        if (!p.fw || p.fwm) {
            TimedLaunch tl(K_GEN, s);
            if (rq_launch_gen(ga, s) != hipSuccess) return RQ_EHIP;
        }
        // merge
        if (p.mrg && (rc = launch_merge(p, merge_args(g, p, out, ch, ga, kn), ch, s))) return rc;
        // order
        const SweepArgs sa = sweep_args(g, p, b, out, ch, ga, kn);
        if (p.order && rq_launch_order(sa.mrg_len, ch.C, (int*)(ch.wsb + p.off_ord), s) != hipSuccess)
            return RQ_EHIP;
        // sweep; both queues of this chunk (sweep, scan) zeroed by one memset
        if (hipMemsetAsync(ch.wsb + p.off_wq, 0, 2 * sizeof(int), s) != hipSuccess) return RQ_EHIP;
        {
            TimedLaunch tl(K_SWEEP, s);
            const SweepInst inst = rqh::sweep_inst(p, b->ctrl_kind);
            // 16-byte rows (inst.pk) take the bytes of rows_t and rows_sum, back to back
            const hipError_t e = inst.fused ? rq_launch_sweep_fw(sa, inst, s, p.off_rv - p.off_rt)
                                            : rq_launch_sweep(sa, inst, s);
            if (e != hipSuccess) return RQ_EHIP;
        }
        // scan
        if (p.scan) continue;   // the sweep's waves integrated their own rows
        const ScanArgs sc = scan_args(g, p, out, ch, sa);
        TimedLaunch tl(K_SCAN, s);
        if (rq_launch_scan(sc, p.nK, s) != hipSuccess) return RQ_EHIP;
    }
    return join.done();   // the caller's stream waits for every side stream
}

int rq_timing(int enable)
{
    for (int k = 0; k < K_N; ++k) {
        for (auto& e : g_ev[k]) {
            (void)hipEventDestroy(e.first);
            (void)hipEventDestroy(e.second);
        }
        g_ev[k].clear();
    }
    g_timing = enable != 0;
    return RQ_OK;
}

int rq_timing_read(double* ms, int64_t* launches)
{
    if (!ms || !launches) return RQ_EINVAL;
    for (int k = 0; k < K_N; ++k) {
        double tot = 0.0;
        for (auto& e : g_ev[k]) {
            float f = 0.0f;
            if (hipEventSynchronize(e.second) != hipSuccess) return RQ_EHIP;
            if (hipEventElapsedTime(&f, e.first, e.second) != hipSuccess) return RQ_EHIP;
            tot += f;
        }
        ms[k] = tot;
        launches[k] = (int64_t)g_ev[k].size();
    }
    return rq_timing(g_timing ? 1 : 0);
}

namespace {
// replay workspace: per-df status, pivot rows, fallback sink keys; the large
// layout adds per-df hash tables / sequential-replay state (slots [4 r0, 4 r1))
struct RpPlan {
    size_t off_info, off_dt, off_sum, off_valid, off_cnt, off_keys, off_gkeys, off_gstate, small, large;
    // chunked replay area (RQ_REPLAY_CHUNKED), after the large area when both are asked for
    int64_t max_chunks;
    size_t c_cbase, c_hkeys, c_hdense, c_gstart, c_gbase, c_carry, c_state, chunk;
};
RpPlan rp_plan(int64_t n_rows, int64_t n_df, int32_t nK)
{
    RpPlan p{};
    const size_t A = 256, n = (size_t)std::max<int64_t>(n_rows, 1);
    size_t o = 0;
    p.off_info = o;  o = align_up(o + sizeof(RpInfo) * (size_t)std::max<int64_t>(n_df, 1), A);
    p.off_dt = o;    o = align_up(o + 8 * n, A);
    p.off_sum = o;   o = align_up(o + 8 * n, A);
    p.off_valid = o; o = align_up(o + 4 * n, A);
    p.off_cnt = o;   o = align_up(o + 4 * n * (size_t)nK, A);
    p.off_keys = o;  o = align_up(o + 8 * n, A);
    p.small = o;
    p.off_gkeys = o; o = align_up(o + 8 * 4 * n, A);
    p.off_gstate = o; o = align_up(o + 16 * 4 * n, A);
    p.large = o;
    // chunk area, offsets relative to its start: per df the chunk prefix and a sink hash
    // table; per chunk (<= n_rows / RC_L + n_df) its t-group counts and RC_S carries / states
    const size_t nd = (size_t)std::max<int64_t>(n_df, 1);
    p.max_chunks = std::max<int64_t>(n_rows, 0) / RC_L + std::max<int64_t>(n_df, 1);
    const size_t mc = (size_t)p.max_chunks;
    size_t c = 0;
    p.c_cbase = c;  c = align_up(c + 8 * (nd + 1), A);
    p.c_hkeys = c;  c = align_up(c + 8 * nd * RC_HT, A);
    p.c_hdense = c; c = align_up(c + 4 * nd * RC_HT, A);
    p.c_gstart = c; c = align_up(c + 4 * mc, A);
    p.c_gbase = c;  c = align_up(c + 8 * mc, A);
    p.c_carry = c;  c = align_up(c + sizeof(RcCarry) * mc * RC_S, A);
    p.c_state = c;  c = align_up(c + sizeof(RcState) * mc * RC_S, A);
    p.chunk = c;
    return p;
}

// the sort area of rq_metrics_replay_unsorted, behind the replay workspace: the radix
// sort's scratch (RP_US_SCRATCH B per row) and the t-ordered columns (24 B per row)
struct RpSortPlan {
    size_t off_scratch, off_t, off_col, off_rank, off_prev, off_g, bytes;
};
RpSortPlan rp_sort_plan(int64_t n_rows)
{
    RpSortPlan p{};
    const size_t A = 256, n = (size_t)std::max<int64_t>(n_rows, 1);
    size_t o = 0;
    p.off_scratch = o; o = align_up(o + RP_US_SCRATCH * n, A);
    p.off_t = o;       o = align_up(o + 8 * n, A);
    p.off_col = o;     o = align_up(o + 4 * n, A);
    p.off_rank = o;    o = align_up(o + 4 * n, A);
    p.off_prev = o;    o = align_up(o + 4 * n, A);
    p.off_g = o;       o = align_up(o + 4 * n, A);
    p.bytes = o;
    return p;
}

// sort_area: null, or the sort area (rp_sort_plan) -- dataframes whose t decreases are
// then evaluated by the sort route instead of being flagged RQ_EUNSORTED
int rp_run(const double* t, const int64_t* src, const int64_t* sink, const int64_t* event_id,
           const int64_t* df_off, int64_t n_df, int64_t n_rows, int64_t src_id, double end_time,
           const int32_t* Ks, int32_t nK, double* out, int64_t* counts, void* workspace,
           size_t workspace_bytes, void* hip_stream, char* sort_area = nullptr)
{
    if (!out || !counts || !workspace || !Ks || n_df < 1 || n_rows < 0) return RQ_EINVAL;
    if (n_rows > 0 && (!t || !src || !sink)) return RQ_EINVAL;
    if (nK < 1 || nK > RQ_MAX_K) return RQ_EINVAL;
    for (int q = 0; q < nK; ++q)
        if (Ks[q] < 1) return RQ_EINVAL;
    const RpPlan p = rp_plan(n_rows, n_df, nK);
    if (workspace_bytes < p.small) return RQ_EINVAL;
    const Knobs kn = rqh::read_knobs();
    // workspace tiers (rq_replay_workspace_size): small [+ large] [+ chunk]
    const bool both = workspace_bytes >= p.large + p.chunk;
    const bool large = workspace_bytes >= p.large;
    const bool has_chunk = both || (!large && workspace_bytes >= p.small + p.chunk);
    char* ws = (char*)workspace;
    char* cw = ws + (both ? p.large : p.small);
    // one dataframe over many workgroups: few, long dataframes (a batch of many fills the
    // chip with one workgroup each)
    bool chunked = has_chunk && n_df <= 64 && n_rows >= 2 * (int64_t)RC_L * n_df;
    if (kn.rp_chunk.set) chunked = has_chunk && kn.rp_chunk.v != 0;   // A/B only
    RpArgs a{};
    a.t = t;
    a.src = src;
    a.sink = sink;
    a.eid = event_id;
    a.df_off = df_off;
    a.n_df = n_df;
    a.n_rows = n_rows;
    a.src_id = src_id;
    a.end = end_time;
    a.nK = nK;
    for (int q = 0; q < RQ_MAX_K; ++q) a.Ks[q] = q < nK ? Ks[q] : 1;
#ifdef RQ_PHASE_CLOCK
    if (kn.clk_replay) a.clk = phase_clk();
#endif
    a.info = (RpInfo*)(ws + p.off_info);
    a.rows_dt = (double*)(ws + p.off_dt);
    a.rows_sum = (double*)(ws + p.off_sum);
    a.rows_valid = (uint32_t*)(ws + p.off_valid);
    a.rows_cnt = (uint32_t*)(ws + p.off_cnt);
    a.keys = (int64_t*)(ws + p.off_keys);
    a.gkeys = large ? (uint64_t*)(ws + p.off_gkeys) : nullptr;
    a.gstate = large ? (void*)(ws + p.off_gstate) : nullptr;
    a.metrics = out;
    a.counts = counts;
    // the small-table tier (two workgroups per CU) first, for one K; A/B knob RQ_RP_SMALL
    a.first_tier = nK == 1 && kn.rp_small ? 0 : 1;
    if (chunked) {
        a.chunked = 1;
        a.max_chunks = p.max_chunks;
        a.cbase = (int64_t*)(cw + p.c_cbase);
        a.ht_keys = (uint64_t*)(cw + p.c_hkeys);
        a.ht_dense = (int*)(cw + p.c_hdense);
        a.gstart = (int*)(cw + p.c_gstart);
        a.gbase = (int64_t*)(cw + p.c_gbase);
        a.carry = (RcCarry*)(cw + p.c_carry);
        a.state = (RcState*)(cw + p.c_state);
    }
    if (sort_area) {
        const RpSortPlan sp = rp_sort_plan(n_rows);
        a.us_scratch = sort_area + sp.off_scratch;
        a.us_t = (double*)(sort_area + sp.off_t);
        a.us_col = (int*)(sort_area + sp.off_col);
        a.us_rank = (int*)(sort_area + sp.off_rank);
        a.us_prev = (int*)(sort_area + sp.off_prev);
        a.us_g = (int*)(sort_area + sp.off_g);
    }
    hipStream_t s = (hipStream_t)hip_stream;
    {
        TimedLaunch tl(K_REPLAY, s);
        if (chunked && rq_launch_rp(a, RP_PHASE_CHUNK, s) != hipSuccess) return RQ_EHIP;
        if (a.first_tier == 0 && rq_launch_rp(a, RP_PHASE_SMALL, s) != hipSuccess) return RQ_EHIP;
        if (rq_launch_rp(a, RP_PHASE_FAST, s) != hipSuccess) return RQ_EHIP;
        if (large && rq_launch_rp(a, RP_PHASE_GLOBAL, s) != hipSuccess) return RQ_EHIP;
        if (rq_launch_rp(a, RP_PHASE_KEYS, s) != hipSuccess) return RQ_EHIP;
        if (rq_launch_rp(a, RP_PHASE_SEQ, s) != hipSuccess) return RQ_EHIP;
        // always launched (no host read of the flags): workgroups of sorted dataframes leave at once
        if (sort_area && rq_launch_rp_sort(a, s) != hipSuccess) return RQ_EHIP;
        if (sort_area && rq_launch_rp(a, RP_PHASE_SEQ_GIVEN, s) != hipSuccess) return RQ_EHIP;
    }
    TimedLaunch tl(K_SCAN, s);
    return rq_launch_rp(a, RP_PHASE_SCAN, s) == hipSuccess ? RQ_OK : RQ_EHIP;
}
}  // namespace

int rq_replay_workspace_size(int64_t n_rows, int64_t n_df, int32_t nK, int32_t flags, size_t* bytes)
{
    if (!bytes || n_rows < 0 || n_df < 1 || nK < 1 || nK > RQ_MAX_K) return RQ_EINVAL;
    const RpPlan p = rp_plan(n_rows, n_df, nK);
    *bytes = ((flags & RQ_REPLAY_LARGE) ? p.large : p.small) + ((flags & RQ_REPLAY_CHUNKED) ? p.chunk : 0);
    return RQ_OK;
}

int rq_metrics_replay(const double* t, const int64_t* src, const int64_t* sink,
                      const int64_t* event_id, int64_t n_rows, int64_t src_id, double end_time,
                      const int32_t* Ks, int32_t nK, double* out, int64_t* counts, void* workspace,
                      size_t workspace_bytes, void* hip_stream)
{
    return rp_run(t, src, sink, event_id, nullptr, 1, n_rows, src_id, end_time, Ks, nK, out,
                  counts, workspace, workspace_bytes, hip_stream);
}

int rq_metrics_replay_batch(const double* t, const int64_t* src, const int64_t* sink,
                            const int64_t* event_id, const int64_t* df_off, int64_t n_df,
                            int64_t n_rows, int64_t src_id, double end_time, const int32_t* Ks,
                            int32_t nK, double* out, int64_t* counts, void* workspace,
                            size_t workspace_bytes, void* hip_stream)
{
    if (!df_off) return RQ_EINVAL;
    return rp_run(t, src, sink, event_id, df_off, n_df, n_rows, src_id, end_time, Ks, nK, out,
                  counts, workspace, workspace_bytes, hip_stream);
}

int rq_replay_unsorted_workspace_size(int64_t n_rows, int64_t n_df, int32_t nK, int32_t flags, size_t* bytes)
{
    size_t base = 0;
    const int rc = rq_replay_workspace_size(n_rows, n_df, nK, flags, &base);
    if (rc != RQ_OK) return rc;
    *bytes = base + rp_sort_plan(n_rows).bytes;
    return RQ_OK;
}

int rq_metrics_replay_unsorted(const double* t, const int64_t* src, const int64_t* sink,
                               const int64_t* event_id, const int64_t* df_off, int64_t n_df,
                               int64_t n_rows, int64_t src_id, double end_time, const int32_t* Ks,
                               int32_t nK, double* out, int64_t* counts, void* workspace,
                               size_t workspace_bytes, void* hip_stream)
{
    if (!workspace || n_rows < 0 || n_df < 1 || nK < 1 || nK > RQ_MAX_K) return RQ_EINVAL;
    if (!df_off && n_df != 1) return RQ_EINVAL;
    // the replay workspace for the layout the caller asked for (the largest that fits with the
    // sort area behind it), of exactly that size: the sorted dataframes take the tiers and
    // return the bits of rq_metrics_replay_batch
    const RpPlan p = rp_plan(n_rows, n_df, nK);
    const size_t sort_bytes = rp_sort_plan(n_rows).bytes;
    const size_t layouts[4] = {p.large + p.chunk, p.large, p.small + p.chunk, p.small};
    for (size_t base : layouts) {
        if (workspace_bytes < base + sort_bytes) continue;
        return rp_run(t, src, sink, event_id, df_off, n_df, n_rows, src_id, end_time, Ks, nK, out,
                      counts, workspace, base, hip_stream, (char*)workspace + base);
    }
    return RQ_EINVAL;
}

}  // extern "C"

// ============================================================================
// analysis entry points (rq_analysis.hip)
// ============================================================================
namespace {
constexpr size_t kOracleLdsMax = 128 * 1024;
size_t oracle_bits_stride(int64_t n_max) { return (size_t)(n_max + 1) * (size_t)((n_max + 1 + 63) / 64); }
bool oracle_lds(int64_t n_max) { return 2 * (size_t)(n_max + 2) * sizeof(double) <= kOracleLdsMax; }
}  // namespace

extern "C" {

int rq_oracle_workspace_size(int32_t n_inst, int64_t n_max, size_t* bytes)
{
    if (!bytes || n_inst < 0 || n_max < 0 || n_max > 1000000) return RQ_EINVAL;
    size_t b = align_up((size_t)n_inst * oracle_bits_stride(n_max) * sizeof(uint64_t), 256);
    if (!oracle_lds(n_max)) b += (size_t)n_inst * 2 * (size_t)(n_max + 2) * sizeof(double);
    *bytes = std::max<size_t>(b, 256);
    return RQ_OK;
}

int rq_oracle_dp(const double* w, const int64_t* w_off, const double* q, const double* s,
                 int32_t n_inst, int64_t n_max, double* cost, int32_t* events, int32_t* ranks,
                 const int64_t* out_off, void* workspace, size_t workspace_bytes, void* hip_stream)
{
    if (n_inst < 0) return RQ_EINVAL;
    if (n_inst == 0) return RQ_OK;
    if (!w || !w_off || !q || !s || !cost || !events || !ranks || !out_off || !workspace) return RQ_EINVAL;
    size_t need = 0;
    const int rc = rq_oracle_workspace_size(n_inst, n_max, &need);
    if (rc != RQ_OK) return rc;
    if (workspace_bytes < need) return RQ_EINVAL;
    OracleArgs a{};
    a.w = w;
    a.w_off = w_off;
    a.q = q;
    a.s = s;
    a.n_inst = n_inst;
    a.n_max = n_max;
    a.cost = cost;
    a.events = events;
    a.ranks = ranks;
    a.out_off = out_off;
    a.bits = (uint64_t*)workspace;
    a.bits_stride = (int64_t)oracle_bits_stride(n_max);
    a.gcol = (double*)((char*)workspace +
                       align_up((size_t)n_inst * oracle_bits_stride(n_max) * sizeof(uint64_t), 256));
    hipStream_t st = (hipStream_t)hip_stream;
    TimedLaunch tl(K_REPLAY, st);
    return rq_launch_oracle_dp(a, oracle_lds(n_max), st) == hipSuccess ? RQ_OK : RQ_EHIP;
}

int rq_rank_table(const double* t, const int64_t* src, const int32_t* sink_col, int64_t n_rows,
                  int32_t n_cols, int64_t src_id, int32_t fill, int64_t n_t, double* table,
                  double* index, int32_t* err, void* hip_stream)
{
    if (!t || !src || !sink_col || !table || !index || !err) return RQ_EINVAL;
    if (n_rows < 1 || n_cols < 1 || n_t < 1 || n_t > n_rows) return RQ_EINVAL;
    RankTableArgs a{};
    a.t = t;
    a.src = src;
    a.col = sink_col;
    a.n_rows = n_rows;
    a.n_cols = n_cols;
    a.src_id = src_id;
    a.fill = fill ? 1 : 0;
    a.n_t = n_t;
    a.table = table;
    a.index = index;
    a.err = err;
    hipStream_t st = (hipStream_t)hip_stream;
    TimedLaunch tl(K_REPLAY, st);
    return rq_launch_rank_table(a, st) == hipSuccess ? RQ_OK : RQ_EHIP;
}

int rq_u_int(const double* table, const double* index, int64_t n_t, int32_t n_cols,
             const int32_t* fcol, const double* wts, int32_t n_f, double end_time, double* out,
             void* workspace, size_t workspace_bytes, void* hip_stream)
{
    if (!table || !index || !out || !workspace || n_t < 1 || n_cols < 1 || n_f < 0) return RQ_EINVAL;
    if (n_f > 0 && (!fcol || !wts)) return RQ_EINVAL;
    if (workspace_bytes < (size_t)n_t * sizeof(double)) return RQ_EINVAL;
    UIntArgs a{};
    a.table = table;
    a.index = index;
    a.n_t = n_t;
    a.n_cols = n_cols;
    a.fcol = fcol;
    a.wts = wts;
    a.n_f = n_f;
    a.end = end_time;
    a.x = (double*)workspace;
    a.out = out;
    hipStream_t st = (hipStream_t)hip_stream;
    TimedLaunch tl(K_SCAN, st);
    return rq_launch_u_int(a, st) == hipSuccess ? RQ_OK : RQ_EHIP;
}

}  // extern "C"

// ============================================================================
// event-log export (State.get_dataframe at batch scale)
// ============================================================================
extern "C" {

int rq_log_rows(rq_graph_t g, const int32_t* ev_src, const int64_t* counts, int64_t n_rep,
                int64_t ev_cap, int64_t* row_off, void* hip_stream)
{
    if (!g || !ev_src || !counts || !row_off || n_rep < 1 || ev_cap < 1) return RQ_EINVAL;
    LogArgs a{};
    a.ev_src = ev_src;
    a.counts = counts;
    a.n_rep = n_rep;
    a.ev_cap = ev_cap;
    a.csr_ptr = g->d_csr_ptr.p;
    a.n_str = g->n_str;
    a.row_off = row_off;
    hipStream_t st = (hipStream_t)hip_stream;
    TimedLaunch tl(K_REPLAY, st);
    return rq_launch_log_rows(a, st) == hipSuccess ? RQ_OK : RQ_EHIP;
}

int rq_log_expand(rq_graph_t g, const double* ev_t, const int32_t* ev_src, const int64_t* counts,
                  int64_t n_rep, int64_t ev_cap, const int64_t* row_off, int64_t* event_id,
                  double* time_delta, int64_t* src_id, double* t, int64_t* sink_id,
                  void* hip_stream)
{
    if (!g || !ev_t || !ev_src || !counts || !row_off || n_rep < 1 || ev_cap < 1) return RQ_EINVAL;
    if (!event_id || !time_delta || !src_id || !t || !sink_id) return RQ_EINVAL;
    LogArgs a{};
    a.ev_t = ev_t;
    a.ev_src = ev_src;
    a.counts = counts;
    a.n_rep = n_rep;
    a.ev_cap = ev_cap;
    a.csr_ptr = g->d_csr_ptr.p;
    a.csr_col = g->d_csr_col_el.p;
    a.n_str = g->n_str;
    a.src_ids = g->d_src_id.p;
    a.sink_ids = g->d_sink_ids.p;
    a.start = g->start;
    a.row_off = const_cast<int64_t*>(row_off);
    a.event_id = event_id;
    a.time_delta = time_delta;
    a.src_id = src_id;
    a.t = t;
    a.sink_id = sink_id;
    hipStream_t st = (hipStream_t)hip_stream;
    TimedLaunch tl(K_REPLAY, st);
    return rq_launch_log_expand(a, st) == hipSuccess ? RQ_OK : RQ_EHIP;
}

// the LogView of a call on graph g
static LogView log_view(rq_graph_t g, const double* ev_t, const int32_t* ev_src, const int64_t* counts,
                        int64_t n_rep, int64_t ev_cap)
{
    LogView v{};
    v.ev_t = ev_t;
    v.ev_src = ev_src;
    v.counts = counts;
    v.n_rep = n_rep;
    v.ev_cap = ev_cap;
    v.csr_ptr = g->d_csr_ptr.p;
    v.csr_col = g->d_csr_col_el.p;
    v.n_str = g->n_str;
    v.n_sinks = g->n_sinks;
    v.ctrl_idx = g->ctrl_idx;
    v.end = g->end;
    return v;
}

// 1 <= nK <= RQ_MAX_K values K >= 1 into dst; false otherwise
static bool copy_ks(const int32_t* Ks, int32_t nK, int (&dst)[RQ_MAX_K])
{
    if (!Ks || nK < 1 || nK > RQ_MAX_K) return false;
    for (int q = 0; q < nK; ++q) {
        if (Ks[q] < 1) return false;
        dst[q] = Ks[q];
    }
    return true;
}

// What no log kernel plays: duplicate edges give one sink several rows per event
// (fractional pivot cells: the sequential sweep's business), and the per-sink state of a
// replica lives in one wave's LDS, which max_sinks sinks fill.
static bool log_unsupported(rq_graph_t g, int max_sinks) { return g->multi || g->n_sinks > max_sinks; }

int rq_log_timeline(rq_graph_t g, const double* ev_t, const int32_t* ev_src, const int64_t* counts,
                    int64_t n_rep, int64_t ev_cap, const double* edges, int32_t n_bins,
                    const int32_t* Ks, int32_t nK, double* metrics, int64_t* posts,
                    int32_t* wall_posts, int32_t* status, void* hip_stream)
{
    if (!g || !ev_t || !ev_src || !counts || !edges || !metrics || !posts || !status) return RQ_EINVAL;
    if (n_rep < 1 || n_rep > INT32_MAX || ev_cap < 1 || n_bins < 1) return RQ_EINVAL;
    TimelineArgs a{};
    if (!copy_ks(Ks, nK, a.Ks)) return RQ_EINVAL;
    if (log_unsupported(g, RQ_TIMELINE_MAX_SINKS)) return RQ_EUNSUPPORTED;
    a.log = log_view(g, ev_t, ev_src, counts, n_rep, ev_cap);
    a.edges = edges;
    a.n_bins = n_bins;
    a.nK = nK;
    a.metrics = metrics;
    a.posts = posts;
    a.wall_posts = wall_posts;
    a.status = status;
    hipStream_t st = (hipStream_t)hip_stream;
    TimedLaunch tl(K_REPLAY, st);
    return rq_launch_timeline(a, st) == hipSuccess ? RQ_OK : RQ_EHIP;
}

int32_t rq_log_followers_max_sinks(int32_t nK, int32_t with_rows)
{
    if (nK < 1 || nK > RQ_MAX_K) return 0;
    return RQ_FOLLOWERS_LDS_BYTES / rq_followers_sink_bytes(nK, with_rows != 0);
}

// What rq_log_followers and rq_log_followers_tiled check first and hand to their kernels;
// each goes on with its own sink limit.
static int followers_args(rq_graph_t g, const double* ev_t, const int32_t* ev_src, const int64_t* counts,
                          int64_t n_rep, int64_t ev_cap, const int32_t* Ks, int32_t nK, double* vals,
                          double* first_t, int32_t* rows, double* r2_true, int32_t* status, FollowersArgs& a)
{
    if (!g || !ev_t || !ev_src || !counts || !vals || !first_t || !r2_true || !status) return RQ_EINVAL;
    // ev_cap <= 2^24 bounds every rank, so rank^2 < 2^48 and the replica's sum stays in int64
    if (n_rep < 1 || n_rep > INT32_MAX || ev_cap < 1 || ev_cap > (1 << 24)) return RQ_EINVAL;
    if (!copy_ks(Ks, nK, a.Ks)) return RQ_EINVAL;
    a.log = log_view(g, ev_t, ev_src, counts, n_rep, ev_cap);
    a.nK = nK;
    a.vals = vals;
    a.first_t = first_t;
    a.rows = rows;
    a.r2_true = r2_true;
    a.status = status;
    return RQ_OK;
}

int rq_log_followers(rq_graph_t g, const double* ev_t, const int32_t* ev_src, const int64_t* counts,
                     int64_t n_rep, int64_t ev_cap, const int32_t* Ks, int32_t nK, double* vals,
                     double* first_t, int32_t* rows, double* r2_true, int32_t* status, void* hip_stream)
{
    FollowersArgs a{};
    const int rc = followers_args(g, ev_t, ev_src, counts, n_rep, ev_cap, Ks, nK, vals, first_t, rows, r2_true,
                                  status, a);
    if (rc != RQ_OK) return rc;
    if (log_unsupported(g, rq_log_followers_max_sinks(nK, rows != nullptr))) return RQ_EUNSUPPORTED;
    hipStream_t st = (hipStream_t)hip_stream;
    TimedLaunch tl(K_REPLAY, st);
    return rq_launch_followers(a, st) == hipSuccess ? RQ_OK : RQ_EHIP;
}

int32_t rq_log_followers_tile_sinks(void) { return RQ_FOLLOWERS_TILE_SINKS; }

int rq_log_followers_tiled_workspace(rq_graph_t g, int64_t n_rep, size_t* bytes)
{
    if (!g || !bytes || n_rep < 1 || n_rep > INT32_MAX) return RQ_EINVAL;
    if (log_unsupported(g, RQ_FOLLOWERS_TILED_MAX_SINKS)) return RQ_EUNSUPPORTED;
    *bytes = rqh::followers_tiled_ws_bytes(g->n_sinks, n_rep);
    return RQ_OK;
}

int rq_log_followers_tiled(rq_graph_t g, const double* ev_t, const int32_t* ev_src, const int64_t* counts,
                           int64_t n_rep, int64_t ev_cap, const int32_t* Ks, int32_t nK, double* vals,
                           double* first_t, int32_t* rows, double* r2_true, int32_t* status, void* workspace,
                           size_t workspace_bytes, void* hip_stream)
{
    FollowersTiledArgs a{};
    const int rc = followers_args(g, ev_t, ev_src, counts, n_rep, ev_cap, Ks, nK, vals, first_t, rows, r2_true,
                                  status, a.f);
    if (rc != RQ_OK) return rc;
    if (!workspace) return RQ_EINVAL;
    if (log_unsupported(g, RQ_FOLLOWERS_TILED_MAX_SINKS)) return RQ_EUNSUPPORTED;
    // one block per (replica, tile) on the grid's x axis
    if (n_rep * (int64_t)g->n_tiles > INT32_MAX) return RQ_EINVAL;
    if (workspace_bytes < rqh::followers_tiled_ws_bytes(g->n_sinks, n_rep)) return RQ_EINVAL;
    a.tile_ptr = g->d_tile_ptr.p;
    a.tile_col = g->d_tile_col.p;
    a.n_tiles = g->n_tiles;
    a.flags = static_cast<int32_t*>(workspace);
    hipStream_t st = (hipStream_t)hip_stream;
    TimedLaunch tl(K_REPLAY, st);
    return rq_launch_followers_tiled(a, st) == hipSuccess ? RQ_OK : RQ_EHIP;
}

int rq_log_rank_hist(rq_graph_t g, const double* ev_t, const int32_t* ev_src, const int64_t* counts,
                     int64_t n_rep, int64_t ev_cap, const double* edges, int32_t n_bins, int32_t n_ranks,
                     double* hist, int32_t* n_seen, int32_t* max_rank, int32_t* status, void* hip_stream)
{
    if (!g || !ev_t || !ev_src || !counts || !edges || !hist || !n_seen || !max_rank || !status) return RQ_EINVAL;
    if (n_rep < 0 || n_rep > INT32_MAX || ev_cap < 0 || n_bins < 1 || n_ranks < 1 ||
        n_ranks > RQ_RANK_HIST_MAX_RANKS)
        return RQ_EINVAL;
    if (log_unsupported(g, RQ_TIMELINE_MAX_SINKS)) return RQ_EUNSUPPORTED;
    if (n_rep == 0) return RQ_OK;   // nothing to play, nothing to write
    RankHistArgs a{};
    a.log = log_view(g, ev_t, ev_src, counts, n_rep, ev_cap);
    a.edges = edges;
    a.n_bins = n_bins;
    a.n_ranks = n_ranks;
    a.hist = hist;
    a.n_seen = n_seen;
    a.max_rank = max_rank;
    a.status = status;
    hipStream_t st = (hipStream_t)hip_stream;
    TimedLaunch tl(K_REPLAY, st);
    return rq_launch_rank_hist(a, st) == hipSuccess ? RQ_OK : RQ_EHIP;
}

// the blocks of an rq_log_metrics launch: one per replica up to RQ_LM_SLOTS
static int64_t log_metrics_slots(int64_t n_rep) { return n_rep < RQ_LM_SLOTS ? n_rep : RQ_LM_SLOTS; }

// what rq_log_metrics and its workspace query refuse alike; slim: the entries on 8-byte cells,
// which differ in the sink limit and the LDS formula only
static int log_metrics_check(rq_graph_t g, int64_t n_rep, int64_t ev_cap, int32_t nK, bool slim = false)
{
    if (!g || n_rep < 1 || n_rep > INT32_MAX || ev_cap < 1) return RQ_EINVAL;
    if (nK < 1 || nK > RQ_MAX_K) return RQ_EINVAL;
    if (log_unsupported(g, slim ? RQ_LOG_METRICS_SLIM_MAX_SINKS : RQ_LOG_METRICS_MAX_SINKS)) return RQ_EUNSUPPORTED;
    // a cell counts a column's rows in a t-group in 24 bits and sums their ranks in 40: logs
    // with room for more events are not played here (the dataframe replay takes any)
    if (ev_cap > RQ_LM_MAX_EV_CAP) return RQ_EUNSUPPORTED;
    // the stream bits share the cells' LDS: past ~1.2 million streams they outgrow it
    const size_t lds = slim ? rq_log_metrics_slim_lds_bytes(g->n_sinks, g->n_str)
                            : rq_log_metrics_lds_bytes(g->n_sinks, g->n_str);
    if (lds > RQ_LM_LDS_BYTES) return RQ_EUNSUPPORTED;
    return RQ_OK;
}

// a block's slot of the workspace: its pivot rows and, behind them, the slim cells' spill words
static size_t log_metrics_slot(rq_graph_t g, int64_t ev_cap, int32_t nK, bool slim)
{
    return slim ? rq_log_metrics_slim_slot_bytes(ev_cap, nK, g->n_sinks) : rq_log_metrics_slot_bytes(ev_cap, nK);
}

// what both cell layouts hand their kernels once the call is accepted
static void log_metrics_fill(LogMetricsArgs& a, rq_graph_t g, const double* ev_t, const int32_t* ev_src,
                             const int64_t* counts, int64_t n_rep, int64_t ev_cap, int32_t nK, double* metrics,
                             int64_t* out_counts, int32_t* status, void* workspace, bool slim)
{
    a.log = log_view(g, ev_t, ev_src, counts, n_rep, ev_cap);
    a.nK = nK;
    a.state_bytes = slim ? rq_log_metrics_slim_state_bytes(g->n_sinks, g->n_str)
                         : rq_log_metrics_state_bytes(g->n_sinks, g->n_str);
    a.spill_off = slim ? rq_log_metrics_slot_bytes(ev_cap, nK) : 0;
    a.rows = static_cast<char*>(workspace);
    a.metrics = metrics;
    a.out_counts = out_counts;
    a.status = status;
}

static int log_metrics_workspace(rq_graph_t g, int64_t n_rep, int64_t ev_cap, int32_t nK, size_t* bytes, bool slim)
{
    if (!bytes) return RQ_EINVAL;
    const int rc = log_metrics_check(g, n_rep, ev_cap, nK, slim);
    if (rc != RQ_OK) return rc;
    *bytes = (size_t)log_metrics_slots(n_rep) * log_metrics_slot(g, ev_cap, nK, slim);
    return RQ_OK;
}

static int log_metrics_run(rq_graph_t g, const double* ev_t, const int32_t* ev_src, const int64_t* counts,
                           int64_t n_rep, int64_t ev_cap, const int32_t* Ks, int32_t nK, double* metrics,
                           int64_t* out_counts, int32_t* status, void* workspace, size_t workspace_bytes,
                           void* hip_stream, bool slim)
{
    if (!g || !ev_t || !ev_src || !counts || !metrics || !out_counts || !status || !workspace) return RQ_EINVAL;
    LogMetricsArgs a{};
    if (!copy_ks(Ks, nK, a.Ks)) return RQ_EINVAL;
    const int rc = log_metrics_check(g, n_rep, ev_cap, nK, slim);
    if (rc != RQ_OK) return rc;
    a.n_slots = (int)log_metrics_slots(n_rep);
    a.slot_bytes = log_metrics_slot(g, ev_cap, nK, slim);
    if (workspace_bytes < (size_t)a.n_slots * a.slot_bytes || (reinterpret_cast<uintptr_t>(workspace) & 7))
        return RQ_EINVAL;
    log_metrics_fill(a, g, ev_t, ev_src, counts, n_rep, ev_cap, nK, metrics, out_counts, status, workspace, slim);
    hipStream_t st = (hipStream_t)hip_stream;
    TimedLaunch tl(K_REPLAY, st);
    return rq_launch_log_metrics(a, st, slim) == hipSuccess ? RQ_OK : RQ_EHIP;
}

int rq_log_metrics_workspace(rq_graph_t g, int64_t n_rep, int64_t ev_cap, int32_t nK, size_t* bytes)
{
    return log_metrics_workspace(g, n_rep, ev_cap, nK, bytes, false);
}

int rq_log_metrics(rq_graph_t g, const double* ev_t, const int32_t* ev_src, const int64_t* counts,
                   int64_t n_rep, int64_t ev_cap, const int32_t* Ks, int32_t nK, double* metrics,
                   int64_t* out_counts, int32_t* status, void* workspace, size_t workspace_bytes,
                   void* hip_stream)
{
    return log_metrics_run(g, ev_t, ev_src, counts, n_rep, ev_cap, Ks, nK, metrics, out_counts, status, workspace,
                           workspace_bytes, hip_stream, false);
}

int rq_log_metrics_slim_workspace(rq_graph_t g, int64_t n_rep, int64_t ev_cap, int32_t nK, size_t* bytes)
{
    return log_metrics_workspace(g, n_rep, ev_cap, nK, bytes, true);
}

int rq_log_metrics_slim(rq_graph_t g, const double* ev_t, const int32_t* ev_src, const int64_t* counts,
                        int64_t n_rep, int64_t ev_cap, const int32_t* Ks, int32_t nK, double* metrics,
                        int64_t* out_counts, int32_t* status, void* workspace, size_t workspace_bytes,
                        void* hip_stream)
{
    return log_metrics_run(g, ev_t, ev_src, counts, n_rep, ev_cap, Ks, nK, metrics, out_counts, status, workspace,
                           workspace_bytes, hip_stream, true);
}

// the blocks of an rq_log_metrics_of launch: one per (replica, source) up to the slot count
static int64_t log_of_slots(int64_t n_rep, int32_t n_src)
{
    const int slots = std::min(rqh::read_knobs().lm_of_slots, RQ_LM_SLOTS);
    return rqh::log_of_blocks(n_rep, n_src, slots);
}

static int log_metrics_of_workspace(rq_graph_t g, int32_t n_src, int64_t n_rep, int64_t ev_cap, int32_t nK,
                                    size_t* bytes, bool slim)
{
    if (!bytes || n_src < 1 || n_src > RQ_LOG_OF_MAX_SRC) return RQ_EINVAL;
    const int rc = log_metrics_check(g, n_rep, ev_cap, nK, slim);
    if (rc != RQ_OK) return rc;
    *bytes = (size_t)log_of_slots(n_rep, n_src) * log_metrics_slot(g, ev_cap, nK, slim);
    return RQ_OK;
}

static int log_metrics_of_run(rq_graph_t g, const int64_t* src_ids, int32_t n_src, int32_t scope,
                              const double* ev_t, const int32_t* ev_src, const int64_t* counts, int64_t n_rep,
                              int64_t ev_cap, const int32_t* Ks, int32_t nK, double* metrics, int64_t* out_counts,
                              int32_t* status, void* workspace, size_t workspace_bytes, void* hip_stream, bool slim)
{
    if (!g || !src_ids || !ev_t || !ev_src || !counts || !metrics || !out_counts || !status || !workspace)
        return RQ_EINVAL;
    if (scope != RQ_LOG_OF_DF && scope != RQ_LOG_OF_OWN) return RQ_EINVAL;
    LogMetricsOfArgs b{};
    LogMetricsArgs& a = b.m;
    if (rqh::log_of_streams(*g, src_ids, n_src, b.trk) != RQ_OK) return RQ_EINVAL;
    if (!copy_ks(Ks, nK, a.Ks)) return RQ_EINVAL;
    const int rc = log_metrics_check(g, n_rep, ev_cap, nK, slim);
    if (rc != RQ_OK) return rc;
    a.n_slots = (int)log_of_slots(n_rep, n_src);
    a.slot_bytes = log_metrics_slot(g, ev_cap, nK, slim);
    if (workspace_bytes < (size_t)a.n_slots * a.slot_bytes || (reinterpret_cast<uintptr_t>(workspace) & 7))
        return RQ_EINVAL;
    log_metrics_fill(a, g, ev_t, ev_src, counts, n_rep, ev_cap, nK, metrics, out_counts, status, workspace, slim);
    b.n_src = n_src;
    b.scope = scope;
    hipStream_t st = (hipStream_t)hip_stream;
    TimedLaunch tl(K_REPLAY, st);
    return rq_launch_log_metrics_of(b, st, slim) == hipSuccess ? RQ_OK : RQ_EHIP;
}

int rq_log_metrics_of_workspace(rq_graph_t g, int32_t n_src, int64_t n_rep, int64_t ev_cap, int32_t nK,
                                size_t* bytes)
{
    return log_metrics_of_workspace(g, n_src, n_rep, ev_cap, nK, bytes, false);
}

int rq_log_metrics_of(rq_graph_t g, const int64_t* src_ids, int32_t n_src, int32_t scope, const double* ev_t,
                      const int32_t* ev_src, const int64_t* counts, int64_t n_rep, int64_t ev_cap,
                      const int32_t* Ks, int32_t nK, double* metrics, int64_t* out_counts, int32_t* status,
                      void* workspace, size_t workspace_bytes, void* hip_stream)
{
    return log_metrics_of_run(g, src_ids, n_src, scope, ev_t, ev_src, counts, n_rep, ev_cap, Ks, nK, metrics,
                              out_counts, status, workspace, workspace_bytes, hip_stream, false);
}

int rq_log_metrics_of_slim_workspace(rq_graph_t g, int32_t n_src, int64_t n_rep, int64_t ev_cap, int32_t nK,
                                     size_t* bytes)
{
    return log_metrics_of_workspace(g, n_src, n_rep, ev_cap, nK, bytes, true);
}

int rq_log_metrics_of_slim(rq_graph_t g, const int64_t* src_ids, int32_t n_src, int32_t scope, const double* ev_t,
                           const int32_t* ev_src, const int64_t* counts, int64_t n_rep, int64_t ev_cap,
                           const int32_t* Ks, int32_t nK, double* metrics, int64_t* out_counts, int32_t* status,
                           void* workspace, size_t workspace_bytes, void* hip_stream)
{
    return log_metrics_of_run(g, src_ids, n_src, scope, ev_t, ev_src, counts, n_rep, ev_cap, Ks, nK, metrics,
                              out_counts, status, workspace, workspace_bytes, hip_stream, true);
}

int rq_log_game_workspace(rq_graph_t g, int32_t n_players, size_t* bytes)
{
    if (!g || !bytes || n_players < 1) return RQ_EINVAL;
    if (n_players > RQ_GAME_MAX_PLAYERS) return RQ_EUNSUPPORTED;
    *bytes = rqh::game_ws_bytes(g->n_str, n_players);
    return RQ_OK;
}

int32_t rq_log_game_table_in_lds(rq_graph_t g, int32_t n_players)
{
    if (!g || n_players < 1 || n_players > RQ_GAME_MAX_PLAYERS) return 0;
    return rqh::game_table_in_lds(g->n_str, n_players) ? 1 : 0;
}

// the players' tables [inv | meta | lane_stream | lane_col] to the workspace, through the
// graph's pinned ring (stage_tables' protocol: the copy is truly asynchronous)
static int stage_game(rq_graph* g, const rqh::GameTables& t, char* ws, hipStream_t s)
{
    const size_t bytes = rqh::game_ws_bytes(g->n_str, t.P);
    std::lock_guard<std::mutex> lk(g->stage_mu);
    Stage* slot = nullptr;
    const int rc = stage_slot(g, bytes, &slot);
    if (rc != RQ_OK) return rc;
    Stage& st = *slot;
    char* tab = (char*)st.buf;
    std::memset(tab, 0, bytes);
    const size_t off_l = rqh::game_ws_off_lanes(g->n_str, t.P);
    std::memcpy(tab, t.inv.data(), t.inv.size() * sizeof(double));
    std::memcpy(tab + rqh::game_ws_off_meta(g->n_str, t.P), t.meta.data(), t.meta.size() * sizeof(int));
    std::memcpy(tab + off_l, t.lane_stream.data(), t.lane_stream.size() * sizeof(int));
    std::memcpy(tab + off_l + 256, t.lane_col.data(), t.lane_col.size() * sizeof(int));
    if (hipMemcpyAsync(ws, tab, bytes, hipMemcpyHostToDevice, s) != hipSuccess ||
        hipEventRecord(st.done, s) != hipSuccess)
        return RQ_EHIP;
    return RQ_OK;
}

int rq_log_game(rq_graph_t g, const rq_game_player* players, int32_t n_players, const uint32_t* seeds,
                const double* ev_t, const int32_t* ev_src, const int64_t* counts, int64_t n_rep,
                int64_t ev_cap, int64_t max_events, double* out_t, int32_t* out_src, int64_t out_cap,
                int64_t* out_counts, int64_t* player_posts, int32_t* status, void* workspace,
                size_t workspace_bytes, void* hip_stream)
{
    if (!g || !players || !seeds || !ev_t || !ev_src || !counts || !out_t || !out_src || !out_counts ||
        !player_posts || !status || !workspace)
        return RQ_EINVAL;
    if (n_rep < 1 || n_rep > INT32_MAX || ev_cap < 0 || out_cap < 1) return RQ_EINVAL;
    rqh::GameTables t;
    const int rc = rqh::game_tables(*g, players, n_players, &t);
    if (rc != RQ_OK) return rc;
    if (workspace_bytes < rqh::game_ws_bytes(g->n_str, t.P)) return RQ_EINVAL;
    hipStream_t st = (hipStream_t)hip_stream;
    char* ws = static_cast<char*>(workspace);
    const int rs = stage_game(g, t, ws, st);
    if (rs != RQ_OK) return rs;
    GameArgs a{};
    a.ev_t = ev_t;
    a.ev_src = ev_src;
    a.counts = counts;
    a.n_rep = n_rep;
    a.ev_cap = ev_cap;
    a.max_events = max_events;
    a.n_str = g->n_str;
    a.P = t.P;
    a.ctrl_lane = t.ctrl_lane;
    a.ctrl_idx = g->ctrl_idx;
    a.inv = reinterpret_cast<const double*>(ws);
    a.meta = reinterpret_cast<const int*>(ws + rqh::game_ws_off_meta(g->n_str, t.P));
    a.lane_stream = reinterpret_cast<const int*>(ws + rqh::game_ws_off_lanes(g->n_str, t.P));
    a.lane_col = a.lane_stream + 64;
    a.in_lds = rqh::game_table_in_lds(g->n_str, t.P) ? 1 : 0;
    a.seeds = seeds;
    a.start = g->start;
    a.end = g->end;
    a.out_t = out_t;
    a.out_src = out_src;
    a.out_cap = out_cap;
    a.out_counts = out_counts;
    a.player_posts = player_posts;
    a.status = status;
    TimedLaunch tl(K_SWEEP, st);
    return rq_launch_game(a, st) == hipSuccess ? RQ_OK : RQ_EHIP;
}

}  // extern "C"

extern "C" int rq_phase_clock(unsigned long long* host8)
{
    // RQ_PHASE_CLOCK diagnostic builds only: copy out and clear the per-phase
    // s_memtime sums of every rq_sweep_fw wave since the last call
    if (!host8) return RQ_EINVAL;
    for (int q = 0; q < 8; ++q) host8[q] = 0;
    if (!g_clk) return RQ_EUNSUPPORTED;
    if (hipDeviceSynchronize() != hipSuccess ||
        hipMemcpy(host8, g_clk, 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemset(g_clk, 0, 8 * sizeof(unsigned long long)) != hipSuccess)
        return RQ_EHIP;
    return RQ_OK;
}

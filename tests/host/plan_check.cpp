// plan_check.cpp -- the host core of librq (redqueen_amd/csrc/rq_host.h) without a GPU:
// graph builder, planner and controller tables, built with the system compiler under
// ASan + UBSan by tests/test_plan_host_cpu.py.  No HIP: the three device queries are
// defined here (no occupancy, 256 CUs), so the planner takes its LDS bound.
//
// Every expectation is a value an existing GPU test pins (tests/test_gpu_graphs.py,
// tests/test_gpu_sweep_scan.py: variant and sources per lane only -- ring depth and column
// placement move with occupancy), a size include/rq.h or rq_host.h documents, or
// arithmetic written out below; none comes from a run of the planner.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <initializer_list>
#include <string>
#include <utility>
#include <vector>

#include "../../redqueen_amd/csrc/rq_host.h"

int rq_sweep_blocks_per_cu(const SweepInst&, int, size_t) { return 0; }
int rq_fw_blocks_per_cu(const SweepInst&, int, size_t) { return 0; }
int rq_cu_count() { return 256; }

using namespace rqh;

static int g_fail = 0, g_checks = 0;
static std::string g_case;
#define CHECK(c)                                                                            \
    do {                                                                                    \
        ++g_checks;                                                                         \
        if (!(c)) {                                                                         \
            ++g_fail;                                                                       \
            std::printf("FAIL %s:%d [%s] %s\n", __FILE__, __LINE__, g_case.c_str(), #c);    \
        }                                                                                   \
    } while (0)

template <class T>
static bool eq(const std::vector<T>& a, std::initializer_list<T> b) { return a == std::vector<T>(b); }

// ---- worlds, through the ABI's descriptor structs ----
struct World {
    int64_t ctrl = 0;
    double T = 0.0;
    std::vector<int64_t> sinks, es, ek;   // sink ids; edge sources / sinks in edge-list order
    std::vector<rq_source_desc> src;
    std::vector<int> arr_of;                // source -> its entry of arr, or -1
    std::vector<std::vector<double>> arr;   // RealData times
    std::vector<double> ctrl_a;             // the controlled slot's replayed times
    void edge(int64_t s, int64_t k) { es.push_back(s); ek.push_back(k); }
    void source(int kind, int64_t id, double p0, double p1 = 0.0, double p2 = 0.0)
    {
        rq_source_desc s{};
        s.kind = kind;
        s.src_id = id;
        s.seed = (uint32_t)id;
        s.p0 = p0; s.p1 = p1; s.p2 = p2;
        src.push_back(s);
        arr_of.push_back(-1);
    }
    void realdata(int64_t id, std::vector<double> t)
    {
        source(RQ_SRC_REALDATA, id, 0.0);
        arr_of.back() = (int)arr.size();
        arr.push_back(std::move(t));
    }
    int build(GraphTopo* g)
    {
        for (size_t k = 0; k < src.size(); ++k)
            if (arr_of[k] >= 0) {
                src[k].n_arr = (int32_t)arr[arr_of[k]].size();
                src[k].a = arr[arr_of[k]].data();
            }
        rq_graph_desc d{};
        d.n_sources = (int32_t)src.size();
        d.sources = src.data();
        d.n_sinks = (int32_t)sinks.size();
        d.sink_ids = sinks.data();
        d.n_edges = (int64_t)es.size();
        d.edge_src = es.data();
        d.edge_sink = ek.data();
        d.ctrl_src_id = ctrl;
        d.start_time = 0.0;
        d.end_time = T;
        d.ctrl_n_arr = (int32_t)ctrl_a.size();
        d.ctrl_a = ctrl_a.empty() ? nullptr : ctrl_a.data();
        return topo_build(&d, g);
    }
};

// the README network (redqueen_amd/graphs.py readme())
static World readme()
{
    World w;
    w.ctrl = 1;
    w.T = 100.0;
    w.sinks = {1, 2, 3};
    w.source(RQ_SRC_POISSON2, 2, 10.0);
    w.source(RQ_SRC_HAWKES, 3, 10.0, 1.0, 10.0);
    w.edge(1, 1); w.edge(1, 3); w.edge(2, 1); w.edge(2, 2); w.edge(2, 3); w.edge(3, 3);
    return w;
}

// n_src Poisson2 walls of `deg` distinct sinks each; the controlled source 0 follows the
// first n_fol sinks (the shape of _many_sources / _wide in tests/test_gpu_graphs.py)
static World many(int n_src, int n_sinks = 120, int deg = 3, int n_fol = 30, double T = 6.0, double rate = 0.4)
{
    World w;
    w.ctrl = 0;
    w.T = T;
    for (int x = 1; x <= n_sinks; ++x) w.sinks.push_back(x);
    for (int f = 1; f <= n_fol; ++f) w.edge(0, f);
    for (int k = 0; k < n_src; ++k) {
        w.source(RQ_SRC_POISSON2, 1000 + k, rate);
        for (int i = 0; i < deg; ++i) w.edge(1000 + k, 1 + (int)(((int64_t)k * deg + i) % n_sinks));
    }
    return w;
}

// a RedQueen batch on g: q = 1, s = 1 at every grid point
struct Batch {
    rq_batch_desc b{};
    std::vector<double> q, s;
    std::vector<int32_t> Ks;
    Batch(const GraphTopo& g, std::initializer_list<int32_t> ks, int64_t n_rep, int n_grid = 1)
        : q(n_grid, 1.0), s((size_t)n_grid * std::max(1, g.n_fol), 1.0), Ks(ks)
    {
        b.ctrl_kind = RQ_SRC_OPT;
        b.n_grid = n_grid;
        b.q = q.data();
        b.s = s.data();
        b.n_rep = n_rep;
        b.Ks = Ks.data();
        b.nK = (int32_t)Ks.size();
        b.max_events = -1;
        b.cap_scale = 1.0;
    }
    Batch(const Batch&) = delete;
};

// ---- properties of every plan ----
struct Region {
    const char* name;
    size_t off, bytes;
    size_t end() const { return off + bytes; }
};
static bool disjoint(const Region& a, const Region& b)
{
    return !a.bytes || !b.bytes || a.end() <= b.off || b.end() <= a.off;
}

static void check_layout(const GraphTopo& g, const rq_batch_desc& b, const Plan& p)
{
    const size_t n = (size_t)g.n_str, G = (size_t)b.n_grid;
    const size_t S = b.ctrl_kind == RQ_SRC_OPTPW ? (size_t)b.n_seg : 0;
    // the parameter tables at the start of the workspace: 8-byte entries 8-aligned
    const std::vector<Region> tab = {
        {"inv_c", p.off_invc, 8 * G * n},   {"st_off", p.off_stoff, 8 * n},
        {"rep_idx", p.off_repidx, b.rep_idx ? 8 * (size_t)p.R : 0},
        {"pw_c", p.off_pwc, 8 * G * n * S}, {"pw_max", p.off_pwmax, S ? 8 * G * n : 0},
        {"cap", p.off_cap, 4 * n},          {"rd_k", p.off_rdk, 4 * n}};
    for (size_t i = 0; i < tab.size(); ++i) {
        CHECK(tab[i].end() <= p.tables_bytes);
        CHECK(tab[i].off % (i < 5 ? 8 : 4) == 0);
        for (size_t j = i + 1; j < tab.size(); ++j) CHECK(disjoint(tab[i], tab[j]));
    }
    CHECK(p.tables_bytes <= p.off_set0);
    CHECK(p.off_set0 % 256 == 0 && p.set_stride % 256 == 0);
    // one buffer set: offsets relative to its base, 256-byte aligned
    const size_t C = (size_t)p.chunk, rows = C * (size_t)p.cap_rows;
    const size_t strm = p.fw && !p.fwm ? 0 : C;   // the generating fused sweep keeps its arrivals in LDS
    const size_t subc = p.mrg && p.n_grp > 1 ? C * p.n_grp : 0, sub = subc * (size_t)p.sub_stride;
    const size_t mrg = (p.mrg ? C : 0) * (size_t)p.mrg_stride;
    const std::vector<Region> set = {
        {"rows_t", p.off_rt, 8 * rows},      {"rows_sum", p.off_rs, 8 * rows},
        {"rows_valid", p.off_rv, 4 * rows},  {"rows_cnt", p.off_rc, 4 * rows * p.nK},
        {"streams", p.off_streams, 8 * strm * (size_t)p.capsum},
        {"slen", p.off_slen, 4 * strm * n},  {"sub_t", p.off_sub_t, 8 * sub},
        {"sub_j", p.off_sub_j, 2 * sub},     {"sub_len", p.off_sub_len, 4 * subc},
        {"mrg_t", p.off_mt, 8 * mrg},        {"mrg_j", p.off_mj, 2 * mrg},
        {"mrg_jh", p.off_mjh, n > 65535 ? mrg : 0},
        {"mrg_len", p.off_mlen, 4 * (p.mrg ? C : 0)},
        {"order", p.off_ord, 4 * (p.order ? C : 0)},
        {"sall", p.off_sall, 4 * C},         {"wq", p.off_wq, 8}};
    // the one intended alias: the per-source streams are dead once merged and may lie over
    // the pivot rows (set[0..3]) -- inside them, never across their end
    const bool alias = p.mrg && p.off_streams < set[3].end() && set[4].end() > set[0].off;
    if (alias) CHECK(p.off_streams >= set[0].off && set[4].end() <= set[3].end());
    for (size_t i = 0; i < set.size(); ++i) {
        CHECK(set[i].off % 256 == 0);
        CHECK(set[i].end() <= p.set_stride);
        for (size_t j = i + 1; j < set.size(); ++j)
            if (!(alias && j == 4 && i < 4)) CHECK(disjoint(set[i], set[j]));
    }
    if (subc)   // a first-level group's sequence holds all of its streams' arrivals
        for (int q = 0; q < p.n_grp; ++q) {
            int64_t c = 0;
            for (int j = q * p.grp_sz; j < std::min(g.n_str, (q + 1) * p.grp_sz); ++j) c += p.cap[j];
            CHECK(c <= p.sub_stride);
        }
    // nbuf sets, then the sequential sweep's global per-sink slots
    CHECK(p.nbuf >= 1 && p.nbuf <= 3);
    CHECK(p.off_set0 + (size_t)p.nbuf * p.set_stride <= p.off_gs);
    CHECK(p.off_gs % 256 == 0);
    CHECK(p.off_gs + (p.gs ? (size_t)p.gs_slots * (size_t)p.gs_stride : 0) <= p.total);
    if (p.gs) CHECK(p.gs_slots >= 1 && (size_t)p.gs_stride >= 16 * ((size_t)g.n_sinks + 1));
}

static void check_plan(const GraphTopo& g, const rq_batch_desc& b, const Plan& p, double budget)
{
    check_layout(g, b, p);
    // chunking
    CHECK(p.chunk >= 1 && p.chunk <= p.R);
    const int64_t nch = (p.R + p.chunk - 1) / p.chunk;
    if (p.nbuf == 2) CHECK(nch % 2 == 0);
    if (b.chunk <= 0 && budget > 0.0) CHECK((double)p.total <= budget);
    // capacities
    int64_t sum = 0;
    CHECK((int)p.cap.size() == g.n_str && (int)p.st_off.size() == g.n_str);
    for (int j = 0; j < g.n_str; ++j) {
        CHECK(p.cap[j] % 16 == 0 && p.cap[j] >= 0);
        CHECK(p.st_off[j] == sum);
        sum += p.cap[j];
    }
    CHECK(p.capsum == sum);
    CHECK(p.cap_rows % 32 == 0 && p.cap_rows >= 64);
    CHECK(p.mrg_stride <= p.capsum);
    if (b.max_events >= 0) CHECK(p.cap_rows <= (std::max<int64_t>(64, b.max_events + 1) + 31) / 32 * 32);
}

// plan batch b on g without knobs and without a budget, check it, return the nine
// rq_plan_info_n values
struct Info {
    int rc = 0;
    int64_t v[9] = {0};
    Plan p;
    int64_t variant() const { return v[0]; }
    int64_t per_lane() const { return v[1]; }
    int64_t scan() const { return v[8]; }
};
static Info plan(const GraphTopo& g, const rq_batch_desc& b, const Knobs& kn = Knobs(), double budget = 0.0)
{
    Info i;
    i.rc = make_plan(g, &b, kn, budget, &i.p);
    if (i.rc == RQ_OK) {
        check_plan(g, b, i.p, budget);
        plan_info(i.p, b.ctrl_kind, i.v);
    }
    return i;
}
static bool sequential(const Info& i) { return i.variant() == 1 || i.variant() == 4; }

// ---- the graph builder and the controller tables on a six-edge graph ----
static World six_edges()
{
    World w;
    w.ctrl = 5;
    w.T = 10.0;
    w.sinks = {30, 10, 20};                  // columns: 10 -> 0, 20 -> 1, 30 -> 2
    w.source(RQ_SRC_POISSON2, 9, 1.0);       // static
    w.source(RQ_SRC_POISSON, 2, 2.0);        // dynamic
    w.realdata(8, {4.0, 6.0});               // static; shares t = 4 with source 3
    w.realdata(3, {1.0, 4.0, 11.0});         // 11 > end_time: dropped
    w.edge(9, 20); w.edge(5, 20); w.edge(2, 10); w.edge(9, 10); w.edge(5, 10); w.edge(3, 30);
    return w;
}

static void test_builder()
{
    g_case = "six edges";
    World w = six_edges();
    GraphTopo g;
    CHECK(w.build(&g) == RQ_OK);
    CHECK(g.n_str == 5 && g.n_sinks == 3 && g.n_edges == 6 && g.n_fol == 2);
    CHECK(eq<int64_t>(g.sink_ids, {10, 20, 30}));
    // dynamic streams first, then the static ones (the controlled slot among them), by id
    CHECK(eq<int64_t>(g.src_id, {2, 3, 5, 8, 9}));
    CHECK(eq<int>(g.is_static, {0, 1, 1, 1, 1}));
    CHECK(g.ctrl_idx == 2);
    CHECK(eq<int>(g.orig_idx, {1, 3, -1, 2, 0}));
    CHECK(eq<int>(g.kind, {RQ_SRC_POISSON, RQ_SRC_REALDATA, RQ_SRC_NONE, RQ_SRC_REALDATA, RQ_SRC_POISSON2}));
    CHECK(eq<int>(g.arr_off, {0, 0, 2, 2, 4}) && eq<int>(g.arr_n, {0, 2, 0, 2, 0}));
    CHECK(eq<double>(g.arr_a, {1.0, 4.0, 4.0, 6.0}));
    // rows: 2 -> [10]; 3 -> [30]; 5 -> [20, 10], stored as the sorted followers; 8 -> []; 9 -> [20, 10]
    CHECK(eq<int>(g.csr_ptr, {0, 1, 2, 4, 4, 6}));
    CHECK(eq<int>(g.csr_col, {0, 2, 0, 1, 1, 0}));
    CHECK(eq<int>(g.csr_col_el, {0, 2, 1, 0, 1, 0}));
    CHECK(eq<int>(g.lay_ptr, {0, 1, 2, 3, 4, 5}) && eq<int>(g.lay_end, {1, 2, 4, 4, 6}));
    CHECK(!g.multi && !g.ctrl_dup);
    CHECK(eq<int>(g.fol, {0, 1}) && eq<int64_t>(g.fol_ids, {10, 20}));
    CHECK(eq<int>(g.col_to_fol, {0, 1, -1}));
    CHECK(eq<int>(g.outdeg_f, {1, 0, 2, 0, 2}));
    CHECK(g.nw == 1 && eq<uint32_t>(g.masks, {1u, 4u, 3u, 0u, 3u}));
    CHECK(eq<uint32_t>(g.fbits, {3u}));
    // the controller posts first against a static source or a larger id: only 2 < 5 is neither
    CHECK(eq<int>(g.cbf, {0, 1, 1, 1, 1}));
    CHECK(g.rd_ties && g.rd_ties_ctrl);   // t = 4 twice among the walls

    g_case = "six edges, inv_c";
    // c_j = sum over j's edges into followers, edge-list order, of sqrt(s_f / q); followers (10, 20)
    Batch bt(g, {1}, 4, 2);
    bt.q = {1.0, 4.0};
    bt.s = {1.0, 4.0, 9.0, 0.1};
    bt.b.q = bt.q.data();
    bt.b.s = bt.s.data();
    const CtrlTables t = ctrl_tables(g, &bt.b);
    CHECK(t.pwc.empty() && t.pwmax.empty() && t.invc.size() == 10);
    for (int gi = 0; gi < 2; ++gi) {
        const double w10 = std::sqrt(bt.s[2 * gi] / bt.q[gi]), w20 = std::sqrt(bt.s[2 * gi + 1] / bt.q[gi]);
        double c2 = 0.0, c9 = 0.0;
        c2 = c2 + w10;                  // source 2: (2, 10)
        c9 = c9 + w20; c9 = c9 + w10;   // source 9: (9, 20) then (9, 10)
        const double want[5] = {1.0 / c2, 0.0, 0.0, 0.0, 1.0 / c9};   // 3 reaches no follower, 8 nothing
        for (int j = 0; j < 5; ++j) CHECK(t.invc[5 * gi + j] == want[j]);
    }

    g_case = "six edges, no wall tie, replayed controller";
    World v = six_edges();
    v.arr[0] = {5.0, 6.0};     // source 8: no time of source 3
    v.ctrl_a = {6.5, 1.0};     // the controlled slot replays t = 1, as source 3 does
    GraphTopo h;
    CHECK(v.build(&h) == RQ_OK);
    CHECK(!h.rd_ties && h.rd_ties_ctrl);
    CHECK(h.ctrl_arr_n == 2 && h.ctrl_arr_off == 2 && eq<double>(h.arr_a, {1.0, 4.0, 1.0, 6.5, 5.0, 6.0}));

    g_case = "builder refusals";
    World bad = six_edges();
    bad.edge(7, 10);   // unknown source
    GraphTopo x;
    CHECK(bad.build(&x) == RQ_EINVAL);
    World dup = six_edges();
    dup.sinks.push_back(10);   // duplicate sink id
    GraphTopo y;
    CHECK(dup.build(&y) == RQ_EINVAL);
}

// ---- decisions that do not depend on occupancy ----
static void test_decisions()
{
    {
        World w = readme();
        GraphTopo g;
        CHECK(w.build(&g) == RQ_OK);
        g_case = "readme K=(1,)";   // the merged fused sweep on sink bitsets, its own scan
        Batch b1(g, {1}, 8);
        Info i = plan(g, b1.b);
        CHECK(i.rc == RQ_OK && i.variant() >= 20 && i.variant() % 10 == 2 && i.per_lane() == 0 && i.scan() == 1);
        g_case = "readme K=(1,) RQ_SWEEP_SCAN=0";
        Knobs off;
        off.sweep_scan = false;
        CHECK(plan(g, b1.b, off).scan() == 0);
        g_case = "readme K=(1,) sweep_mode 7";   // test_plans_that_keep_the_scan_kernel: 12, no scan
        b1.b.sweep_mode = 7;
        i = plan(g, b1.b);
        CHECK(i.rc == RQ_OK && i.variant() == 12 && i.per_lane() == 1 && i.scan() == 0);
        b1.b.sweep_mode = 0;
        g_case = "readme K=(1,) event log";
        b1.b.flags = RQ_RUN_EVENT_LOG;
        CHECK(plan(g, b1.b).scan() == 0);
        b1.b.flags = 0;
        g_case = "readme K=(1,) max_events 50";
        b1.b.max_events = 50;
        i = plan(g, b1.b);
        CHECK(i.rc == RQ_OK && i.scan() == 0 && i.p.cap_rows == 64);   // max(64, 51) rounded up to 32
        b1.b.max_events = 0;
        CHECK(plan(g, b1.b).scan() == 0);
        g_case = "readme K=(1,2,5)";
        Batch b3(g, {1, 2, 5}, 8);
        i = plan(g, b3.b);
        CHECK(i.rc == RQ_OK && i.variant() == 20 && i.per_lane() == 0 && i.scan() == 1);

        g_case = "readme rep_idx";
        const int64_t ids[3] = {0, 5, 7};
        Batch br(g, {1}, 8);
        br.b.rep_idx = ids;
        br.b.n_local = 3;
        i = plan(g, br.b);
        CHECK(i.rc == RQ_OK && i.p.R == 3);
        CHECK(i.p.off_repidx % 8 == 0 && i.p.off_repidx + 3 * 8 <= i.p.off_pwc && i.p.off_pwc <= i.p.tables_bytes);
        const int64_t bad[3] = {0, 8, 7};   // 8 is outside n_grid x n_rep
        br.b.rep_idx = bad;
        CHECK(plan(g, br.b).rc == RQ_EINVAL);

        g_case = "readme, duplicated wall edge";   // a multigraph: the sequential sweep
        World m = readme();
        m.edge(2, 1);
        GraphTopo gm;
        CHECK(m.build(&gm) == RQ_OK && gm.multi && !gm.ctrl_dup);
        Batch bm(gm, {1, 2}, 3);
        i = plan(gm, bm.b);
        CHECK(i.rc == RQ_OK && sequential(i));
        g_case = "readme, duplicated controlled edge";
        World c = readme();
        c.edge(1, 1);
        GraphTopo gc;
        CHECK(c.build(&gc) == RQ_OK && gc.ctrl_dup && gc.n_fol == 2);
        Batch bc(gc, {1}, 1);
        CHECK(plan(gc, bc.b).rc == RQ_EINVAL);
        bc.b.ctrl_kind = RQ_SRC_NONE;   // refused for the RedQueen controllers only
        CHECK(plan(gc, bc.b).rc == RQ_OK);
    }
    for (int n_src : {65, 100}) {
        g_case = "windowed sweep, " + std::to_string(n_src) + " sources";
        World w = many(n_src);
        GraphTopo g;
        CHECK(w.build(&g) == RQ_OK);
        Batch b(g, {1, 2}, 6);
        b.b.sweep_mode = 6;
        const Info i = plan(g, b.b);
        CHECK(i.rc == RQ_OK && i.variant() == 0 && i.per_lane() == 2);
    }
    {
        g_case = "600 sources, sequential";
        World w = many(600);
        GraphTopo g;
        CHECK(w.build(&g) == RQ_OK);
        Batch b(g, {1, 2}, 4);
        b.b.sweep_mode = 2;
        Info i = plan(g, b.b);
        CHECK(i.rc == RQ_OK && sequential(i) && i.per_lane() == 16);
        g_case = "600 sources, fast";   // test_more_than_512_sources: merged streams
        b.b.sweep_mode = 0;
        i = plan(g, b.b);
        CHECK(i.rc == RQ_OK && !sequential(i) && i.per_lane() == 0);
    }
    {
        g_case = "2100 sources, sequential";
        World w = many(2100);
        GraphTopo g;
        CHECK(w.build(&g) == RQ_OK);
        Batch b(g, {1, 2}, 4);
        b.b.sweep_mode = 2;
        const Info i = plan(g, b.b);
        CHECK(i.rc == RQ_OK && sequential(i) && i.per_lane() == 0);
    }
    {
        g_case = "513 sources";   // 514 streams in groups of 64: ceil(514 / 64) = 9
        World w = many(513);
        GraphTopo g;
        CHECK(w.build(&g) == RQ_OK && g.n_str == 514);
        Batch b(g, {1, 2}, 4);
        const Info i = plan(g, b.b);
        CHECK(i.rc == RQ_OK && i.p.mrg && i.p.n_grp == 9 && i.p.grp_sz == 64 && i.per_lane() == 0);
    }
    {
        g_case = "70000 sinks K=(1,)";   // per-wave LDS sink bits on merged streams
        World w = many(40, 70000, 60, 400, 4.0, 1.5);
        GraphTopo g;
        CHECK(w.build(&g) == RQ_OK && g.nw == 0);
        Batch b(g, {1}, 6);
        const Info i = plan(g, b.b);
        CHECK(i.rc == RQ_OK && i.variant() % 10 == 3 && i.per_lane() == 0);
    }
}

// ---- chunking within a budget ----
static void test_budget()
{
    World w = many(50, 1000, 5, 1000, 100.0, 1.0);   // C3's size
    GraphTopo g;
    CHECK(w.build(&g) == RQ_OK);
    g_case = "budget: one chunk";
    Batch one(g, {1}, 10000);
    one.b.chunk = 10000;   // the caller's chunk: one launch, whatever it takes
    const Info i1 = plan(g, one.b);
    CHECK(i1.rc == RQ_OK && i1.p.chunk == 10000 && i1.p.nbuf == 1);
    g_case = "budget: library chunking";
    Batch b(g, {1}, 10000);
    Info i = plan(g, b.b);
    CHECK(i.rc == RQ_OK && i.p.nbuf == 2 && i.p.chunk == 5000);   // include/rq.h: an even number of chunks
    for (double budget : {(double)i1.p.total - 1.0, (double)i1.p.total / 3.0, 64.0 * (1 << 20)}) {
        g_case = "budget " + std::to_string((long long)budget);
        i = plan(g, b.b, Knobs(), budget);   // check_plan: total <= budget
        CHECK(i.rc == RQ_OK || i.rc == RQ_ENOMEM);
        if (i.rc == RQ_OK) CHECK(i.p.chunk < 10000);
    }
    g_case = "budget of one byte";   // no replica fits: the shrink loop ends at chunk 1
    CHECK(plan(g, b.b, Knobs(), 1.0).rc == RQ_ENOMEM);
    g_case = "budget ignored for a caller's chunk";
    i = plan(g, one.b, Knobs(), 1.0);
    CHECK(i.rc == RQ_OK && i.p.chunk == 10000);

    g_case = "OptPWSignificance, 4 segments";
    Batch pw(g, {1, 2}, 100, 2);
    std::vector<double> s_pw((size_t)2 * g.n_fol * 4, 1.5);
    pw.b.ctrl_kind = RQ_SRC_OPTPW;
    pw.b.n_seg = 4;
    pw.b.period = 100.0;
    pw.b.s_pw = s_pw.data();
    i = plan(g, pw.b);
    CHECK(i.rc == RQ_OK && i.scan() == 0);
    const CtrlTables t = ctrl_tables(g, &pw.b);
    CHECK(t.pwc.size() == (size_t)2 * g.n_str * 4 && t.pwmax.size() == (size_t)2 * g.n_str);
    CHECK(t.pwc.size() * 8 + i.p.off_pwc <= i.p.off_pwmax && t.pwmax.size() * 8 + i.p.off_pwmax <= i.p.tables_bytes);
}

int main()
{
    test_builder();
    test_decisions();
    test_budget();
    std::printf("%d checks, %d failed\n", g_checks, g_fail);
    return g_fail ? 1 : 0;
}

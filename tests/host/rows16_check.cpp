// rows16_check.cpp -- when the planner gives the merged fused sweep 16-byte row records
// (Plan.rows16, redqueen_amd/csrc/rq_host.h), at the edges of the record's fields: 65,535
// sinks (valid and cnt are 16 bits) and n_sinks x mrg_stride = 2^32 (sumR is 32 bits).  Host
// code only, built with the system compiler by tests/test_rows16_host_cpu.py; the three
// device queries are defined here, so the planner takes its LDS bound.
//
// The expectations are arithmetic on the plan's own n_sinks and mrg_stride, written out
// below; none comes from a run of the planner's condition.
#include <cstdio>
#include <string>
#include <vector>

#include "../../redqueen_amd/csrc/rq_host.h"

int rq_sweep_blocks_per_cu(const SweepInst&, int, size_t) { return 0; }
int rq_fw_blocks_per_cu(const SweepInst&, int, size_t) { return 0; }
int rq_cu_count() { return 256; }

using namespace rqh;

static int g_fail = 0, g_checks = 0;
static std::string g_case;
#define CHECK(c)                                                                         \
    do {                                                                                 \
        ++g_checks;                                                                      \
        if (!(c)) {                                                                      \
            ++g_fail;                                                                    \
            std::printf("FAIL %s:%d [%s] %s\n", __FILE__, __LINE__, g_case.c_str(), #c); \
        }                                                                                \
    } while (0)

// n_src Poisson2 walls at `rate` over [0, T], each reaching `deg` sinks; the controlled
// source 0 follows the first n_fol sinks
struct World {
    std::vector<int64_t> sinks, es, ek;
    std::vector<rq_source_desc> src;
    double T;
    World(int n_src, int n_sinks, int deg, int n_fol, double T_, double rate) : T(T_)
    {
        for (int x = 1; x <= n_sinks; ++x) sinks.push_back(x);
        for (int f = 1; f <= n_fol; ++f) { es.push_back(0); ek.push_back(f); }
        for (int k = 0; k < n_src; ++k) {
            rq_source_desc s{};
            s.kind = RQ_SRC_POISSON2;
            s.src_id = 1000 + k;
            s.seed = (uint32_t)k;
            s.p0 = rate;
            src.push_back(s);
            for (int i = 0; i < deg; ++i) {
                es.push_back(1000 + k);
                ek.push_back(1 + (int)(((int64_t)k * deg + i) % n_sinks));
            }
        }
    }
    int build(GraphTopo* g)
    {
        rq_graph_desc d{};
        d.n_sources = (int32_t)src.size();
        d.sources = src.data();
        d.n_sinks = (int32_t)sinks.size();
        d.sink_ids = sinks.data();
        d.n_edges = (int64_t)es.size();
        d.edge_src = es.data();
        d.edge_sink = ek.data();
        d.ctrl_src_id = 0;
        d.start_time = 0.0;
        d.end_time = T;
        return topo_build(&d, g);
    }
};

struct Batch {
    rq_batch_desc b{};
    std::vector<double> q, s;
    std::vector<int32_t> Ks;
    Batch(const GraphTopo& g, std::vector<int32_t> ks, int64_t n_rep) : q(1, 1.0), s((size_t)g.n_fol, 1.0), Ks(ks)
    {
        b.ctrl_kind = RQ_SRC_OPT;
        b.n_grid = 1;
        b.q = q.data();
        b.s = s.data();
        b.n_rep = n_rep;
        b.Ks = Ks.data();
        b.nK = (int32_t)Ks.size();
        b.max_events = -1;
        b.cap_scale = 1.0;
    }
};

static const uint64_t TWO32 = (uint64_t)1 << 32;

int main()
{
    // ---- the condition itself, at its edges ----
    g_case = "rows16_fits";
    CHECK(rows16_fits(1, 65535, 65537));        // 65535 x 65537 = 2^32 - 1
    CHECK(!rows16_fits(1, 65535, 65538));       // 2^32 + 65534
    CHECK(!rows16_fits(1, 65536, 16));          // valid = 65536 does not fit 16 bits
    CHECK(rows16_fits(1, 65535, 16));
    CHECK(rows16_fits(1, 65536 / 2, 131071));   // 2^15 x (2^17 - 1) = 2^32 - 2^15
    CHECK(!rows16_fits(1, 65536 / 2, 131072));  // 2^32 exactly
    CHECK(rows16_fits(1, 1, (int64_t)TWO32 - 1) && !rows16_fits(1, 1, (int64_t)TWO32));
    CHECK(rows16_fits(1, 0, (int64_t)1 << 20));   // no sink: every field stays 0
    CHECK(!rows16_fits(2, 3, 100) && !rows16_fits(4, 3, 100));   // one K only
    CHECK(!rows16_fits(1, 1000, (int64_t)1 << 62));   // the product is taken in 64 bits, no wrap to a small value
    CHECK(!rows16_fits(1, 65535, ((int64_t)1 << 48) + 1));

    // ---- the planner: 2000 sinks on sink bits, sumR's edge at 2^32 / 2000 = 2,147,483 entries ----
    for (double rate : {300.0, 500.0}) {
        g_case = "2000 sinks, rate " + std::to_string((int)rate);
        World w(50, 2000, 60, 2000, 100.0, rate);
        GraphTopo g;
        CHECK(w.build(&g) == RQ_OK && g.n_sinks == 2000 && g.nw == 63);
        Batch b(g, {1}, 8);
        Plan p;
        CHECK(make_plan(g, &b.b, Knobs(), 0.0, &p) == RQ_OK);
        CHECK(p.fwm && p.scan && p.bits);
        // 50 streams x rate x 100: 1.5 M wall events a replica at rate 300, 2.5 M at 500
        CHECK(rate == 300.0 ? p.mrg_stride < 2147483 : p.mrg_stride > 2147483);
        CHECK(p.rows16 == ((uint64_t)g.n_sinks * (uint64_t)p.mrg_stride < TWO32));
        CHECK(p.rows16 == (rate == 300.0));
        CHECK(sweep_inst(p, RQ_SRC_OPT).pk == p.rows16);
        if (rate == 300.0) {
            // the overflow rerun's doubled capacities: the plan decides again, on its own mrg_stride
            Plan p2;
            b.b.cap_scale = 2.0;
            CHECK(make_plan(g, &b.b, Knobs(), 0.0, &p2) == RQ_OK);
            CHECK(p2.mrg_stride > 2147483 && p2.scan && !p2.rows16);
            b.b.cap_scale = 1.0;
            // the records lie in the bytes of rows_t and rows_sum, back to back: 16 bytes a row
            CHECK(p.off_rs == p.off_rt + 8 * (size_t)p.chunk * (size_t)p.cap_rows);
            CHECK(p.off_rv - p.off_rt >= 16 * (size_t)p.chunk * (size_t)p.cap_rows && p.off_rt % 256 == 0);
            // RQ_ROWS_PACKED=0 and what it must not move
            Knobs off;
            off.rows_packed = false;
            Plan q;
            CHECK(make_plan(g, &b.b, off, 0.0, &q) == RQ_OK);
            CHECK(!q.rows16 && q.scan && q.total == p.total && q.chunk == p.chunk && q.cap_rows == p.cap_rows &&
                  q.off_rt == p.off_rt && q.off_rs == p.off_rs && q.off_rv == p.off_rv && q.off_rc == p.off_rc &&
                  q.set_stride == p.set_stride && q.g_total == p.g_total && q.gwpb == p.gwpb);
            // no scan of its own, no records
            Knobs ns;
            ns.sweep_scan = false;
            CHECK(make_plan(g, &b.b, ns, 0.0, &q) == RQ_OK && !q.scan && !q.rows16);
            b.b.flags = RQ_RUN_EVENT_LOG;
            CHECK(make_plan(g, &b.b, Knobs(), 0.0, &q) == RQ_OK && !q.scan && !q.rows16);
            b.b.flags = 0;
            Batch b2(g, {1, 2}, 8);
            CHECK(make_plan(g, &b2.b, Knobs(), 0.0, &q) == RQ_OK && q.scan && !q.rows16);
        }
    }
    // ---- the planner: 65,535 and 65,536 sinks on columns (one K > 1) ----
    for (int n_sinks : {65535, 65536}) {
        g_case = std::to_string(n_sinks) + " sinks";
        World w(8, n_sinks, 40, 100, 4.0, 1.0);
        GraphTopo g;
        CHECK(w.build(&g) == RQ_OK && g.n_sinks == n_sinks);
        Batch b(g, {2}, 8);
        Plan p;
        CHECK(make_plan(g, &b.b, Knobs(), 0.0, &p) == RQ_OK);
        CHECK(p.fwm && p.scan && !p.bits);
        CHECK((uint64_t)n_sinks * (uint64_t)p.mrg_stride < TWO32);   // a few hundred entries a replica
        CHECK(p.rows16 == (n_sinks == 65535));
        CHECK(p.gcol16 == (n_sinks == 65535 ? 1 : 0));
    }
    std::printf("%d checks, %d failed\n", g_checks, g_fail);
    return g_fail ? 1 : 0;
}

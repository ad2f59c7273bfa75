// tile_check.cpp -- the sink-tiled CSR of the host core (GraphTopo.tile_ptr / tile_col,
// redqueen_amd/csrc/rq_host.h, built by topo_build for rq_log_followers_tiled) without a
// GPU: built with the system compiler under ASan + UBSan by
// tests/test_followers_tiled_cpu.py.  No HIP: the three device queries are defined here.
//
// Graphs of TS - 1, TS, TS + 1, 2 TS and 2 TS + 1 sinks with shuffled sink ids and a
// shuffled edge list.  The expectation of every (tile, stream) row comes from the world's
// own edge list, not from the builder's CSR.
#include <algorithm>
#include <cstdio>
#include <map>
#include <random>
#include <string>
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

static const int TS = RQ_FOLLOWERS_TILE_SINKS;

struct World {
    int n = 0;
    std::vector<int64_t> sinks, es, ek;
    std::vector<rq_source_desc> src;
    std::map<int64_t, std::vector<int>> fan;   // source id -> its sink columns
    static int64_t id_of(int col) { return 5 + 3 * (int64_t)col; }   // ascending in the column
    void edge(int64_t s, int col)
    {
        es.push_back(s);
        ek.push_back(id_of(col));
        fan[s].push_back(col);
    }
    int build(GraphTopo* g, std::mt19937& rng)
    {
        std::vector<size_t> perm(es.size());
        for (size_t k = 0; k < perm.size(); ++k) perm[k] = k;
        std::shuffle(perm.begin(), perm.end(), rng);
        std::vector<int64_t> s2, k2;
        for (size_t k : perm) { s2.push_back(es[k]); k2.push_back(ek[k]); }
        std::shuffle(sinks.begin(), sinks.end(), rng);
        rq_graph_desc d{};
        d.n_sources = (int32_t)src.size();
        d.sources = src.data();
        d.n_sinks = (int32_t)sinks.size();
        d.sink_ids = sinks.data();
        d.n_edges = (int64_t)s2.size();
        d.edge_src = s2.data();
        d.edge_sink = k2.data();
        d.ctrl_src_id = 1;
        d.start_time = 0.0;
        d.end_time = 10.0;
        return topo_build(&d, g);
    }
};

// controlled source 1: every third sink; 2: every sink; 3: no edge; 4: the last sinks only
// (all in the last tile); 5: 64 columns below the tile 0 / 1 boundary and up to 65 above; 6: a
// random third of the sinks
static World world(int n, std::mt19937& rng)
{
    World w;
    w.n = n;
    for (int c = 0; c < n; ++c) w.sinks.push_back(World::id_of(c));
    for (int64_t id = 2; id <= 6; ++id) {
        rq_source_desc s{};
        s.kind = RQ_SRC_POISSON2;
        s.src_id = id;
        s.seed = (uint32_t)id;
        s.p0 = 1.0;
        w.src.push_back(s);
    }
    for (int c = 0; c < n; c += 3) w.edge(1, c);
    for (int c = 0; c < n; ++c) w.edge(2, c);
    const int last0 = (n - 1) / TS * TS;   // first column of the last tile
    for (int c = std::max(last0, n - 5); c < n; ++c) w.edge(4, c);
    for (int c = std::max(0, TS - 64); c < std::min(n, TS + 65); ++c) w.edge(5, c);
    for (int c = 0; c < n; ++c)
        if (rng() % 3 == 0) w.edge(6, c);
    return w;
}

static void check_tiles(const World& w, const GraphTopo& g)
{
    const int nt = (w.n + TS - 1) / TS;
    CHECK(g.n_tiles == nt);
    CHECK(g.n_str == 6 && g.n_edges == (int64_t)w.es.size());
    const size_t stride = (size_t)g.n_str + 1;
    CHECK(g.tile_ptr.size() == nt * stride);
    CHECK(g.tile_col.size() == (size_t)g.n_edges);
    if (g.tile_ptr.size() != nt * stride || g.tile_col.size() != (size_t)g.n_edges) return;
    // pointers: from 0, monotone, a tile ends where the next begins, the last at n_edges
    CHECK(g.tile_ptr[0] == 0);
    for (int i = 0; i < nt; ++i) {
        for (int j = 0; j < g.n_str; ++j) CHECK(g.tile_ptr[i * stride + j] <= g.tile_ptr[i * stride + j + 1]);
        if (i + 1 < nt) CHECK(g.tile_ptr[i * stride + g.n_str] == g.tile_ptr[(i + 1) * stride]);
    }
    CHECK(g.tile_ptr[(nt - 1) * stride + g.n_str] == (int)g.n_edges);
    bool empty_stream = false, last_only = false;
    for (int j = 0; j < g.n_str; ++j) {
        std::vector<int> full;   // the world's row of stream j
        auto it = w.fan.find(g.src_id[j]);
        if (it != w.fan.end()) full = it->second;
        std::sort(full.begin(), full.end());
        empty_stream = empty_stream || full.empty();
        last_only = last_only || (!full.empty() && full.front() / TS == nt - 1);
        std::vector<int> all;    // the tile rows, tile after tile
        for (int i = 0; i < nt; ++i) {
            const int p0 = g.tile_ptr[i * stride + j], p1 = g.tile_ptr[i * stride + j + 1];
            if (p0 < 0 || p1 > (int)g.n_edges || p0 > p1) { CHECK(false); continue; }
            std::vector<int> row(g.tile_col.begin() + p0, g.tile_col.begin() + p1), exp;
            std::sort(row.begin(), row.end());
            for (int c : full)
                if (c >= i * TS && c < std::min((i + 1) * TS, w.n)) exp.push_back(c);
            CHECK(row == exp);   // exactly the full row's columns inside the tile
            all.insert(all.end(), row.begin(), row.end());
        }
        CHECK(all == full);      // ascending tiles of sorted rows: the rows partition the full row
        // and the builder's own full CSR row holds the same set
        std::vector<int> csr(g.csr_col_el.begin() + g.csr_ptr[j], g.csr_col_el.begin() + g.csr_ptr[j + 1]);
        std::sort(csr.begin(), csr.end());
        CHECK(csr == full);
    }
    CHECK(empty_stream && last_only);
}

int main()
{
    std::mt19937 rng(20240607u);
    for (int n : {TS - 1, TS, TS + 1, 2 * TS, 2 * TS + 1}) {
        if (n < 1) continue;   // TS = 1
        g_case = "sinks " + std::to_string(n);
        World w = world(n, rng);
        GraphTopo g;
        CHECK(w.build(&g, rng) == RQ_OK);
        CHECK(!g.multi);
        check_tiles(w, g);
    }
    {
        g_case = "duplicate edge";
        World w = world(TS + 1, rng);
        w.edge(2, 7);
        GraphTopo g;
        CHECK(w.build(&g, rng) == RQ_OK);
        CHECK(g.multi && g.n_tiles == 0 && g.tile_ptr.empty() && g.tile_col.empty());
    }
    {
        g_case = "sink limit";
        for (int n : {RQ_FOLLOWERS_TILED_MAX_SINKS, RQ_FOLLOWERS_TILED_MAX_SINKS + 1}) {
            World w = world(n, rng);
            GraphTopo g;
            CHECK(w.build(&g, rng) == RQ_OK);
            if (n <= RQ_FOLLOWERS_TILED_MAX_SINKS) check_tiles(w, g);
            else CHECK(g.n_tiles == 0 && g.tile_ptr.empty() && g.tile_col.empty());
        }
    }
    {
        g_case = "constants and workspace";
        // every nK / rows variant of a tile fits 160 KiB: 12 + 8 (4 + 2) + 8 = 68 bytes a sink
        CHECK(TS >= 1 && (long long)TS * 68 <= 163840 && TS <= 2409);
        CHECK(RQ_FOLLOWERS_TILED_MAX_SINKS == 40960 && RQ_FOLLOWERS_TILED_MAX_SINKS * 4 == 163840);
        CHECK(followers_tiles(1) == 1 && followers_tiles(TS) == 1 && followers_tiles(TS + 1) == 2);
        CHECK(followers_tiles(2 * TS) == 2 && followers_tiles(2 * TS + 1) == 3);
        // 4 n_rep tiles, rounded up to 256
        CHECK(followers_tiled_ws_bytes(1, 1) == 256 && followers_tiled_ws_bytes(TS, 64) == 256);
        CHECK(followers_tiled_ws_bytes(TS, 65) == 512 && followers_tiled_ws_bytes(TS + 1, 64) == 512);
        CHECK(followers_tiled_ws_bytes(2 * TS + 1, 1000) == 12032);   // 12,000 -> 47 x 256
    }
    std::printf("%d checks, %d failed\n", g_checks, g_fail);
    return g_fail ? 1 : 0;
}

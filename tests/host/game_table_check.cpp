// game_table_check.cpp -- the players' rate tables of rq_log_game (rqh::game_tables,
// redqueen_amd/csrc/rq_host.h) and their refusals without a GPU, built with the system
// compiler under ASan + UBSan by tests/test_game_host_cpu.py.  Only rq_topo.cpp is linked:
// the tables need neither the planner nor HIP.  Every expectation is arithmetic written out
// below; none comes from a run of the code under test.
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "../../redqueen_amd/csrc/rq_host.h"

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

struct World {
    int64_t ctrl = 1;
    std::vector<int64_t> sinks, es, ek;
    std::vector<rq_source_desc> src;
    void edge(int64_t s, int64_t k) { es.push_back(s); ek.push_back(k); }
    void source(int kind, int64_t id, uint32_t flags = 0)
    {
        rq_source_desc s{};
        s.kind = kind;
        s.src_id = id;
        s.flags = flags;
        s.p0 = 1.0; s.p1 = 1.0; s.p2 = 4.0;
        src.push_back(s);
    }
    void player(int64_t id) { source(RQ_SRC_REALDATA, id, RQ_SRCF_DYNAMIC); }   // a replay stream
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
        d.ctrl_src_id = ctrl;
        d.start_time = 0.0;
        d.end_time = 20.0;
        return topo_build(&d, g);
    }
};

// W5 of the game tests: RedQueen 1, Poisson2 2, Hawkes 3, Opts 4 and 5 on sinks 101..103;
// `dup` adds a second (2, 101) edge after (3, 103), `lone` a Poisson2 source 6 on sink 104
// that no player follows
static World w5(bool dup = false, bool lone = false)
{
    World w;
    w.sinks = {101, 102, 103};
    w.source(RQ_SRC_POISSON2, 2);
    w.source(RQ_SRC_HAWKES, 3);
    w.player(4);
    w.player(5);
    for (int64_t k : {101, 102, 103}) w.edge(1, k);
    w.edge(2, 102); w.edge(2, 101);   // out of sink order on purpose
    w.edge(3, 102); w.edge(3, 103);
    if (dup) w.edge(2, 101);
    w.edge(4, 101); w.edge(4, 103);
    w.edge(5, 102);
    if (lone) {
        w.sinks.push_back(104);
        w.source(RQ_SRC_POISSON2, 6);
        w.edge(6, 104);
    }
    return w;
}

static int stream_of(const GraphTopo& g, int64_t id)
{
    for (int j = 0; j < g.n_str; ++j)
        if (g.src_id[j] == id) return j;
    return -1;
}

int main()
{
    const double s1[3] = {1.0, 1.0, 1.0}, s4[2] = {2.0, 0.5}, s5[1] = {1.0};
    const double r5 = std::sqrt(1.0 / 2.0);
    {
        g_case = "W5";
        GraphTopo g;
        World w = w5();
        CHECK(w.build(&g) == RQ_OK);
        // the caller's order is 5, 1, 4: lanes are by src_id, columns remember the caller's
        const rq_game_player pl[3] = {{5, 2.0, s5, 1}, {1, 1.0, s1, 3}, {4, 0.5, s4, 2}};
        GameTables t;
        CHECK(game_tables(g, pl, 3, &t) == RQ_OK);
        CHECK(t.P == 3 && t.ctrl_lane == 0);
        CHECK(t.lane_col == (std::vector<int>{1, 2, 0}));
        CHECK(t.lane_stream == (std::vector<int>{stream_of(g, 1), stream_of(g, 4), stream_of(g, 5)}));
        const int j1 = stream_of(g, 1), j2 = stream_of(g, 2), j3 = stream_of(g, 3), j4 = stream_of(g, 4),
                  j5 = stream_of(g, 5);
        auto C = [&](int lane, int j) { return t.C[(size_t)lane * g.n_str + j]; };
        auto I = [&](int lane, int j) { return t.inv[(size_t)j * t.P + lane]; };
        // lane 0 = player 1: every follower weighs sqrt(1 / 1)
        CHECK(C(0, j1) == 0.0 && C(0, j2) == 2.0 && C(0, j3) == 2.0 && C(0, j4) == 2.0 && C(0, j5) == 1.0);
        // lane 1 = player 4: 101 weighs sqrt(2 / 0.5) = 2, 103 sqrt(0.5 / 0.5) = 1
        CHECK(C(1, j1) == 3.0 && C(1, j2) == 2.0 && C(1, j3) == 1.0 && C(1, j4) == 0.0 && C(1, j5) == 0.0);
        // lane 2 = player 5: 102 weighs sqrt(1 / 2); stream 4 reaches none of its followers
        CHECK(C(2, j1) == r5 && C(2, j2) == r5 && C(2, j3) == r5 && C(2, j4) == 0.0 && C(2, j5) == 0.0);
        CHECK(I(0, j2) == 0.5 && I(0, j1) == 0.0 && I(1, j1) == 1.0 / 3.0 && I(2, j4) == 0.0 && I(2, j3) == 1.0 / r5);
        // ties: a static stream (Poisson2 2, the controlled slot) lets every lane first; the
        // Hawkes source 3 only the lanes of smaller src_id (player 1); player streams by id
        CHECK((t.meta[j2] & 255) == 3 && (t.meta[j1] & 255) == 3 && (t.meta[j3] & 255) == 1);
        CHECK((t.meta[j4] & 255) == 1 && (t.meta[j5] & 255) == 2);
        for (int j = 0; j < g.n_str; ++j) CHECK(t.meta[j] & RQ_GAME_META_EDGE);
    }
    {
        g_case = "multiplicity";
        GraphTopo g;
        World w = w5(true);
        CHECK(w.build(&g) == RQ_OK && g.multi);
        const rq_game_player pl[2] = {{4, 0.5, s4, 2}, {5, 2.0, s5, 1}};
        GameTables t;
        CHECK(game_tables(g, pl, 2, &t) == RQ_OK && t.ctrl_lane == -1);
        const int j2 = stream_of(g, 2);
        // 2's edges in ascending sink id: 101, 101, 102 -> ((0 + 2) + 2) for player 4
        CHECK(t.C[(size_t)0 * g.n_str + j2] == 4.0 && t.inv[(size_t)j2 * 2 + 0] == 0.25);
        CHECK(t.C[(size_t)1 * g.n_str + j2] == r5);
    }
    {
        g_case = "a stream that reaches no follower";
        GraphTopo g;
        World w = w5(false, true);
        CHECK(w.build(&g) == RQ_OK);
        const rq_game_player pl[2] = {{4, 0.5, s4, 2}, {5, 2.0, s5, 1}};
        GameTables t;
        CHECK(game_tables(g, pl, 2, &t) == RQ_OK);
        const int j6 = stream_of(g, 6);
        for (int c = 0; c < 2; ++c) CHECK(t.C[(size_t)c * g.n_str + j6] == 0.0 && t.inv[(size_t)j6 * 2 + c] == 0.0);
    }
    {
        g_case = "64 players, 65 refused";
        World w;
        w.ctrl = 1000;
        w.sinks = {7};
        w.source(RQ_SRC_POISSON, 500);
        w.edge(500, 7);
        for (int64_t k = 0; k < 65; ++k) {
            w.player(k);
            w.edge(k, 7);
        }
        GraphTopo g;
        CHECK(w.build(&g) == RQ_OK);
        const double one[1] = {4.0};
        std::vector<rq_game_player> pl;
        for (int64_t k = 0; k < 65; ++k) pl.push_back({64 - k, 1.0, one, 1});   // descending ids
        GameTables t;
        CHECK(game_tables(g, pl.data(), 64, &t) == RQ_OK && t.P == 64);
        CHECK(t.lane_col[0] == 63 && t.lane_col[63] == 0);   // lane 0 = src_id 1 = the caller's last
        const int jp = stream_of(g, 500);
        for (int c = 0; c < 64; ++c) CHECK(t.inv[(size_t)jp * 64 + c] == 0.5);   // 1 / sqrt(4 / 1)
        CHECK((t.meta[jp] & 255) == 64);   // every player's src_id is below 500
        CHECK(game_tables(g, pl.data(), 65, &t) == RQ_EUNSUPPORTED);
        CHECK(game_ws_bytes(g.n_str, 64) >= (size_t)g.n_str * 64 * 8 + (size_t)g.n_str * 4 + 2 * 64 * 4);
        CHECK(!game_table_in_lds(600, 64) && game_table_in_lds(600, 3) && game_table_in_lds(3000, 2));
    }
    {
        g_case = "refusals";
        GraphTopo g;
        World w = w5();
        w.edge(5, 102);   // a duplicated own edge of player 5
        CHECK(w.build(&g) == RQ_OK);
        GameTables t;
        const rq_game_player ok4[1] = {{4, 0.5, s4, 2}};
        CHECK(game_tables(g, ok4, 1, &t) == RQ_OK);
        const rq_game_player dup5[1] = {{5, 2.0, s5, 1}};
        CHECK(game_tables(g, dup5, 1, &t) == RQ_EINVAL);
        const rq_game_player bad_ns[1] = {{4, 0.5, s4, 1}};
        CHECK(game_tables(g, bad_ns, 1, &t) == RQ_EINVAL);
        const rq_game_player q0[1] = {{4, 0.0, s4, 2}}, qneg[1] = {{4, -1.0, s4, 2}};
        CHECK(game_tables(g, q0, 1, &t) == RQ_EINVAL && game_tables(g, qneg, 1, &t) == RQ_EINVAL);
        const rq_game_player stranger[1] = {{77, 1.0, s4, 2}};
        CHECK(game_tables(g, stranger, 1, &t) == RQ_EINVAL);
        const rq_game_player hawkes[1] = {{3, 1.0, s4, 2}};   // a stream, but not a replay stream
        CHECK(game_tables(g, hawkes, 1, &t) == RQ_EINVAL);
        const rq_game_player twice[2] = {{4, 0.5, s4, 2}, {4, 0.5, s4, 2}};
        CHECK(game_tables(g, twice, 2, &t) == RQ_EINVAL);
        CHECK(game_tables(g, ok4, 0, &t) == RQ_EINVAL);

        g_case = "no followers";
        GraphTopo g2;
        World w2 = w5();
        w2.player(9);   // no edge
        CHECK(w2.build(&g2) == RQ_OK);
        const double none[1] = {1.0};
        const rq_game_player lonely[1] = {{9, 1.0, none, 0}}, lonely1[1] = {{9, 1.0, none, 1}};
        CHECK(game_tables(g2, lonely, 1, &t) == RQ_EINVAL && game_tables(g2, lonely1, 1, &t) == RQ_EINVAL);
    }
    std::printf("%d checks, %d failed\n", g_checks, g_fail);
    return g_fail ? 1 : 0;
}

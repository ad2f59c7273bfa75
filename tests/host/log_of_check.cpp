// log_of_check.cpp -- the tracked sources of rq_log_metrics_of (rqh::log_of_streams and
// rqh::log_of_blocks, redqueen_amd/csrc/rq_host.h) without a GPU, built with the system
// compiler under ASan + UBSan by tests/test_log_sources_cpu.py.  Only rq_topo.cpp is linked.
// Every expectation is written out below; none comes from a run of the code under test.
#include <cstdio>
#include <string>
#include <vector>

#include "../../redqueen_amd/csrc/rq_host.h"

using namespace rqh;

static int g_fail = 0, g_checks = 0;
#define CHECK(c)                                                         \
    do {                                                                 \
        ++g_checks;                                                      \
        if (!(c)) {                                                      \
            ++g_fail;                                                    \
            std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c);      \
        }                                                                \
    } while (0)

int main()
{
    // the controlled source 50 and n wall sources 100 + 3 k, each on sink 7 (and 50 on sink 8)
    const int n = 70;
    std::vector<rq_source_desc> src(n);
    std::vector<int64_t> sinks = {7, 8}, es, ek;
    for (int k = 0; k < n; ++k) {
        src[k] = rq_source_desc{};
        src[k].kind = RQ_SRC_POISSON2;
        src[k].src_id = 100 + 3 * k;
        src[k].p0 = 1.0;
        es.push_back(src[k].src_id);
        ek.push_back(7);
    }
    es.push_back(50);
    ek.push_back(8);
    rq_graph_desc d{};
    d.n_sources = n;
    d.sources = src.data();
    d.n_sinks = 2;
    d.sink_ids = sinks.data();
    d.n_edges = (int64_t)es.size();
    d.edge_src = es.data();
    d.edge_sink = ek.data();
    d.ctrl_src_id = 50;
    d.start_time = 0.0;
    d.end_time = 10.0;
    GraphTopo g;
    CHECK(topo_build(&d, &g) == RQ_OK);
    CHECK(g.n_str == n + 1);

    // every stream, in the graph's order and reversed: trk[k] is the stream of src_ids[k]
    std::vector<int64_t> ids(g.src_id.begin(), g.src_id.begin() + RQ_LOG_OF_MAX_SRC);
    int trk[RQ_LOG_OF_MAX_SRC + 1];
    CHECK(log_of_streams(g, ids.data(), RQ_LOG_OF_MAX_SRC, trk) == RQ_OK);
    for (int k = 0; k < RQ_LOG_OF_MAX_SRC; ++k) CHECK(trk[k] == k);
    std::vector<int64_t> rev(ids.rbegin(), ids.rend());
    CHECK(log_of_streams(g, rev.data(), RQ_LOG_OF_MAX_SRC, trk) == RQ_OK);
    for (int k = 0; k < RQ_LOG_OF_MAX_SRC; ++k) CHECK(trk[k] == RQ_LOG_OF_MAX_SRC - 1 - k);
    // the controlled source is a stream like any other
    const int64_t ctrl = 50;
    CHECK(log_of_streams(g, &ctrl, 1, trk) == RQ_OK);
    CHECK(trk[0] == g.ctrl_idx);

    // refusals
    std::vector<int64_t> all(g.src_id.begin(), g.src_id.end());
    CHECK(log_of_streams(g, all.data(), RQ_LOG_OF_MAX_SRC + 1, trk) == RQ_EINVAL);
    CHECK(log_of_streams(g, all.data(), 0, trk) == RQ_EINVAL);
    CHECK(log_of_streams(g, all.data(), -1, trk) == RQ_EINVAL);
    CHECK(log_of_streams(g, nullptr, 1, trk) == RQ_EINVAL);
    CHECK(log_of_streams(g, all.data(), 1, nullptr) == RQ_EINVAL);
    const int64_t twice[3] = {100, 103, 100}, unknown[2] = {100, 101}, sink_id[1] = {7};
    CHECK(log_of_streams(g, twice, 3, trk) == RQ_EINVAL);
    CHECK(log_of_streams(g, twice, 2, trk) == RQ_OK);
    CHECK(log_of_streams(g, unknown, 2, trk) == RQ_EINVAL);
    CHECK(log_of_streams(g, sink_id, 1, trk) == RQ_EINVAL);

    // blocks: one per (replica, source) up to the slot count
    CHECK(log_of_blocks(1, 1, 4096) == 1);
    CHECK(log_of_blocks(64, 64, 4096) == 4096);
    CHECK(log_of_blocks(63, 65 - 1, 4096) == 63 * 64);
    CHECK(log_of_blocks(65, 64, 4096) == 4096);
    CHECK(log_of_blocks(5, 3, 14) == 14);
    CHECK(log_of_blocks(5, 3, 15) == 15);
    CHECK(log_of_blocks(5, 3, 16) == 15);
    CHECK(log_of_blocks(INT32_MAX, 64, 4096) == 4096);

    std::printf("%d checks, %d failed\n", g_checks, g_fail);
    return g_fail ? 1 : 0;
}

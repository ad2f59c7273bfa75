// rq_log_walk.h -- what the kernels that replay a batch's compact event logs share
// (rq_timeline.hip, rq_followers.hip, rq_rank_hist.hip): the view of the logs and the
// graph, the chunked log reader, the rank rule, the time-bin clipper and the status.
// Each kernel runs one wavefront per replica (the followers' tile kernel: per replica and
// tile of sink columns) and keeps its own per-sink state in LDS.
// rq_followers.hip and rq_rank_hist.hip read their logs through log_walk, and the rank
// histogram clips through BinClip; rq_timeline.hip keeps the same text of both inline,
// where it holds its measured time.
#pragma once
#include "../../include/rq.h"
#include "rq_device.h"

#pragma clang fp contract(off)

// The logs of a batch and the graph they index; first member of every log kernel's args.
struct LogView {
    const double* ev_t;       // [n_rep][ev_cap]
    const int32_t* ev_src;    // [n_rep][ev_cap] stream indices
    const int64_t* counts;    // [n_rep][4], [2] = events
    int64_t n_rep, ev_cap;
    const int* csr_ptr;       // [n_str + 1]
    const int* csr_col;       // sink columns per stream (distinct within a row: no multigraph)
    int n_str, n_sinks, ctrl_idx;
    double end;
};

namespace rq {

struct LogChunk {   // lane l: event k0 + l of the replica (an event past the log, or of a
    double t;       // stream index outside the graph, has an empty row: p0 == p1)
    int j, p0, p1;
};

// Replays replica r's (t, stream) log in order: on_event(t, own, p0, p1, xfirst) once per
// event whose CSR row [p0, p1) is non-empty; own: the controlled source's event; xfirst:
// this lane's sink column of the row's first round (row_sink).  counts[r][2] is clamped
// to [0, ev_cap].  Event times, streams and CSR row bounds are fetched 64 events at a
// time, one chunk ahead; the first 64 sink columns of the next event are fetched while
// the current one is applied.
template <class F>
__device__ __forceinline__ void log_walk(const LogView& v, int64_t r, F&& on_event)
{
    const int lane = lane_id();
    int64_t n = v.counts[r * 4 + 2];
    n = n < 0 ? 0 : (n > v.ev_cap ? v.ev_cap : n);
    const double* T = v.ev_t + r * v.ev_cap;
    const int32_t* J = v.ev_src + r * v.ev_cap;

    auto load_chunk = [&](int64_t k0) {
        LogChunk c;
        c.t = 0.0;
        c.j = -1;
        c.p0 = c.p1 = 0;
        const int64_t k = k0 + lane;
        if (k < n) {
            c.t = T[k];
            const int j = J[k];
            if ((unsigned)j < (unsigned)v.n_str) {
                c.j = j;
                c.p0 = v.csr_ptr[j];
                c.p1 = v.csr_ptr[j + 1];
            }
        }
        return c;
    };

    LogChunk A = load_chunk(0);
    int xcur = 0;
    {
        const int q0 = bcast_i(A.p0, 0), q1 = bcast_i(A.p1, 0);
        if (q0 + lane < q1) xcur = v.csr_col[q0 + lane];
    }
    for (int64_t k0 = 0; k0 < n; k0 += 64) {
        const LogChunk B = load_chunk(k0 + 64);
        const int cnt = (int)((n - k0) < 64 ? (n - k0) : 64);
        for (int i = 0; i < cnt; ++i) {
            const double t = bcast_d(A.t, i);
            const int j = bcast_i(A.j, i);
            const int p0 = bcast_i(A.p0, i), p1 = bcast_i(A.p1, i);
            // the next event's first 64 sink columns, in flight while this one is applied
            const int q0 = i < 63 ? bcast_i(A.p0, i + 1) : bcast_i(B.p0, 0);
            const int q1 = i < 63 ? bcast_i(A.p1, i + 1) : bcast_i(B.p1, 0);
            int xnext = 0;
            if (q0 + lane < q1) xnext = v.csr_col[q0 + lane];
            if (p1 > p0) on_event(t, j == v.ctrl_idx, p0, p1, xcur);
            xcur = xnext;
        }
        A = B;
    }
}

// this lane's sink column in the round of row [p0, p1) that starts at edge e (act: e + lane < p1)
__device__ __forceinline__ int row_sink(const LogView& v, int e, int p0, bool act, int xfirst)
{
    return e == p0 ? xfirst : (act ? v.csr_col[e + lane_id()] : 0);
}

// the controlled source's rank in a sink's feed after a row (rk < 0: no row yet) -- the
// rule of rq_sweep_core.h: an own row sets 0, any other row adds 1 (unseen -> 1)
__device__ __forceinline__ int next_rank(bool own, int rk) { return own ? 0 : (rk < 0 ? 1 : rk + 1); }

__device__ __forceinline__ int32_t log_status(bool have, bool tie)
{
    return tie ? RQ_ST_TIE : (!have ? RQ_ST_EMPTY : 0);
}

// The open time bin b = [e0, e1) of edges[n_bins + 1].  A pivot row holds until the next
// event with an edge, so its integrands f are constant on [cur_t, hi) and the interval is
// clipped to the bins it meets.  Events come in time order: the open bin only moves
// forward, its sums acc live in registers and are stored once, by store(b), when it closes.
struct BinClip {
    const double* edges;
    int nb, b;
    double e0, e1;

    __device__ __forceinline__ BinClip(const double* edges_, int nb_)
        : edges(edges_), nb(nb_), b(0), e0(edges_[0]), e1(edges_[1])
    {
    }

    template <int N, class S>
    __device__ __forceinline__ void close(double (&acc)[N], S&& store)   // store bin b, open b + 1
    {
        store(b);
#pragma unroll
        for (int q = 0; q < N; ++q) acc[q] = 0.0;
        ++b;
        if (b < nb) {
            e0 = edges[b];
            e1 = edges[b + 1];
        }
    }

    // the held row (have: there is one) over [cur_t, hi), then every bin that ends at or
    // before hi closes
    template <int N, class S>
    __device__ __forceinline__ void advance(bool have, double cur_t, double hi, const double (&f)[N],
                                            double (&acc)[N], S&& store)
    {
        while (b < nb) {
            if (have) {
                const double lo = cur_t > e0 ? cur_t : e0;
                const double up = hi < e1 ? hi : e1;
                if (up > lo) {
                    const double len = up - lo;
#pragma unroll
                    for (int q = 0; q < N; ++q) acc[q] = acc[q] + f[q] * len;
                }
            }
            if (!(e1 <= hi)) break;
            close(acc, store);
        }
    }

    // the last row holds until end_time; the bins after it close empty
    template <int N, class S>
    __device__ __forceinline__ void finish(bool have, double cur_t, double end, const double (&f)[N],
                                           double (&acc)[N], S&& store)
    {
        advance(have, cur_t, end, f, acc, store);
        while (b < nb) close(acc, store);
    }
};

}  // namespace rq

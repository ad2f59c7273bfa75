// rq_followers.hip -- per-follower metrics straight from a batch's compact event logs
// (rq_log_followers, rq_log_followers_tiled): for every sink column of
// rank_of_src_in_df's pivot table (utils.py:38-56) the integrals of I(r_i <= K-1), r_i and
// r_i^2 over the column's seen span -- the per-follower terms of the paper's objective and
// of utils.py:84-128 -- plus the sink's first-row time and its own / wall row counts, and
// per replica int_r_2_true (utils.py:124-128), the integral of the row mean of r^2.
//
// One replay (replay<>) in three kernels, one wavefront per block each.  The wave replays a
// replica's (t, stream) log in order (log_walk, rq_log_walk.h) against state private to it in
// LDS, SoA over the columns [x0, x0 + nt) of the graph's sink index, local column x, width W:
//   tlast[x]   f64  time of x's last row                                  (SPANS)
//   acc[q][x]  f64  the NK + 2 running integrals of x                     (SPANS)
//   rank[x]    i32  the controlled source's rank in x's feed (-1: no row yet; next_rank)
//   rows[c][x] i32  own / wall rows of x                                  (SPANS and ROWS)
// Lanes take the event's CSR row 64 sinks per round.
//   SPANS: a sink's rank is constant between two of its rows, so a row at t closes the
// interval [tlast, t) of the rank it replaces: acc_q = acc_q + f_q(rank) * (t - tlast),
// sequentially in time order from 0.0 and with no contraction -- the sum a host loop in the
// same order reproduces bit for bit, whatever columns the wave holds.  A row at tlast itself
// is a duplicate (t, sink) pivot cell (RQ_ST_TIE).  first_t is written when the sink's first
// row plays (NaN at the end for a sink without one), everything else when the log has ended.
//   R2: the replica's pivot row (the state after the last event of a time) enters r2_true as
// sumR2 / nvalid: nvalid seen sinks and the exact integer sumR2 = sum of their rank^2, kept
// up to date per event with a ballot and a wave sum (a wall row adds 2 rank + 1, or 1 for a
// new sink; an own row removes rank^2).  ev_cap <= 2^24 bounds rank^2 below 2^48.  It needs
// every column of the replica in one wave.
//
//   rq_followers_k<NK, ROWS>       SPANS and R2 in one pass over all n_sinks columns, one
//                                  wave per replica: rq_log_followers, graphs whose state
//                                  fits one workgroup's LDS.  Every output element is
//                                  written exactly once.
//   rq_followers_tile_k<NK, ROWS>  SPANS of the columns of one tile of TS sinks
//                                  (RQ_FOLLOWERS_TILE_SINKS), one wave per (replica, tile),
//                                  W = min(TS, n_sinks).  The tile's LogView
//                                  (csr_ptr = tile_ptr + tile (n_str + 1), csr_col =
//                                  tile_col: a CSR of the edges into the tile, GraphTopo)
//                                  makes log_walk replay the whole log and hand over only
//                                  the rows of the wave's own sinks.  Outputs at their places
//                                  of the rq_log_followers layout; lane 0 stores
//                                  flags[r][tile], bit 0 = a sink of the tile got two rows at
//                                  one t.
//   rq_followers_r2_k              R2 on the graph's full CSR, one wave per replica, only
//                                  rank[n_sinks] in LDS (40,960 sinks fill 160 KiB).  After
//                                  the tiles on the caller's stream: it ORs the replica's
//                                  flags, writes status and r2_true and overwrites vals with
//                                  NaN for a TIE / EMPTY replica -- the one place an element
//                                  is written twice.  first_t and rows stay valid.
// No atomics, no zeroing pass, nothing read past a log's count, nothing written outside the
// replica's own output rows, no dependence on the launch geometry.
#include <hip/hip_runtime.h>

#include "rq_device.h"
#include "rq_internal.h"
#include "rq_log_walk.h"

#pragma clang fp contract(off)

using namespace rq;

namespace {

constexpr int TS = RQ_FOLLOWERS_TILE_SINKS;

struct Replayed {
    bool have, tie;   // the log had a row; some sink of the wave's columns got two rows at one t
    double r2acc;     // R2: the replica's int_r_2_true
};

// Replica r's log, seen through v, against the columns [x0, x0 + nt) at LDS width W.  SPANS:
// the per-sink state, written to vals / first_t / rows when the log has ended.  R2: the pivot
// row.  TILED: v may hold rows of other columns; such a lane sits out.  Without it x0 == 0
// and nt == W == n_sinks, and no column is tested.
template <int NK, bool ROWS, bool SPANS, bool R2, bool TILED>
__device__ __forceinline__ Replayed replay(const FollowersArgs& a, const LogView& v, int64_t r, int x0, int nt,
                                           int W)
{
    extern __shared__ __attribute__((aligned(16))) double lds_fl[];
    constexpr int NV = NK + 2;
    const int lane = lane_id();
    const int NS = a.log.n_sinks;
    double* tlast = lds_fl;                                                  // [W]
    double* acc = lds_fl + W;                                                // [NV][W]
    int* rank = reinterpret_cast<int*>(lds_fl + (SPANS ? (size_t)W * (NV + 1) : 0));   // [W]
    int* rown = rank + W;                                                    // [2][W], ROWS only
    for (int x = lane; x < nt; x += 64) {
        if (SPANS) {
            tlast[x] = 0.0;
#pragma unroll
            for (int q = 0; q < NV; ++q) acc[(size_t)q * W + x] = 0.0;
        }
        rank[x] = -1;
        if (SPANS && ROWS) {
            rown[x] = 0;
            rown[W + x] = 0;
        }
    }
    wave_lds_sync();

    double* V = a.vals + (r * NS + x0) * NV;        // the wave's columns of replica r
    double* FT = a.first_t + r * NS + x0;
    int32_t* RW = SPANS && ROWS ? a.rows + (r * NS + x0) * 2 : nullptr;
    int Km1[NK];
    if (SPANS) {
#pragma unroll
        for (int q = 0; q < NK; ++q) Km1[q] = a.Ks[q] - 1;
    }

    // the pivot row that holds: nvalid seen sinks, sumR2 the sum of their squared ranks
    int nvalid = 0;
    int64_t sumR2 = 0;
    bool have = false, tie_l = false;   // tie_l: this lane saw a duplicate (t, sink) cell
    double cur_t = 0.0, r2acc = 0.0;

    // the interval [tlast[x], hi) of the rank rk >= 0 that sink x holds
    auto close_span = [&](int x, int rk, double tl, double hi) {
        const double len = hi - tl;
        if (len > 0.0) {
            const double rho = (double)rk;
#pragma unroll
            for (int q = 0; q < NK; ++q) {
                const double f = rk <= Km1[q] ? 1.0 : 0.0;
                acc[(size_t)q * W + x] = acc[(size_t)q * W + x] + f * len;
            }
            acc[(size_t)NK * W + x] = acc[(size_t)NK * W + x] + rho * len;
            acc[(size_t)(NK + 1) * W + x] = acc[(size_t)(NK + 1) * W + x] + (rho * rho) * len;
        }
    };

    log_walk(v, r, [&](double t, bool own, int p0, int p1, int xfirst) {
        // a new time closes the pivot row that held since cur_t
        if (R2 && have && t != cur_t) r2acc = r2acc + ((double)sumR2 / (double)nvalid) * (t - cur_t);
        have = true;
        cur_t = t;
        int64_t d2 = 0;   // this lane's share of |delta sumR2|, < 2^55
        int dv = 0;
        for (int e = p0; e < p1; e += 64) {
            const bool in = e + lane < p1;
            const int x = row_sink(v, e, p0, in, xfirst) - x0;
            // a column outside the tile cannot come from tile_col; the lane sits out if it does
            const bool act = in && (!TILED || (unsigned)x < (unsigned)nt);
            const int rk = act ? rank[x] : 0;
            if (act) {
                if (rk >= 0) {
                    if (SPANS) {
                        const double tl = tlast[x];
                        if (tl == t) tie_l = true;
                        close_span(x, rk, tl, t);
                    }
                    if (R2) d2 += own ? (int64_t)rk * rk : (int64_t)(2 * rk + 1);
                } else {
                    if (SPANS) FT[x] = t;
                    if (R2 && !own) d2 += 1;
                }
                rank[x] = next_rank(own, rk);
                if (SPANS) tlast[x] = t;
                if (SPANS && ROWS) rown[(own ? 0 : W) + x] = rown[(own ? 0 : W) + x] + 1;
            }
            if (R2) dv += popc(__ballot(act && rk < 0));
        }
        wave_lds_sync();
        if (R2) {
            nvalid += dv;
            const int64_t d = wave_sum_i64(d2);
            sumR2 += own ? -d : d;
        }
    });
    // the last ranks and the last pivot row hold until end_time
    if (R2 && have) r2acc = r2acc + ((double)sumR2 / (double)nvalid) * (v.end - cur_t);
    const bool tie = SPANS && __ballot(tie_l) != 0;
    if (SPANS) {
        for (int x = lane; x < nt; x += 64) {
            const int rk = rank[x];
            if (rk >= 0) close_span(x, rk, tlast[x], v.end);
        }
        wave_lds_sync();

        // a wave that holds the whole replica knows here that it is TIE / EMPTY
        const bool bad = R2 && (tie || !have);
        const double NaN = __builtin_nan("");
        for (int k = lane; k < nt * NV; k += 64) {
            const int x = k / NV, q = k - x * NV;
            V[k] = bad ? NaN : acc[(size_t)q * W + x];
        }
        for (int x = lane; x < nt; x += 64)
            if (rank[x] < 0) FT[x] = NaN;
        if (ROWS)
            for (int k = lane; k < 2 * nt; k += 64) RW[k] = rown[(k & 1) * W + (k >> 1)];
    }
    return {have, tie, r2acc};
}

// the replica's own two outputs, by the wave that ran R2
__device__ __forceinline__ void store_replica(const FollowersArgs& a, int64_t r, bool have, bool tie, double r2acc)
{
    if (lane_id() == 0) {
        a.r2_true[r] = tie || !have ? __builtin_nan("") : r2acc;
        a.status[r] = log_status(have, tie);
    }
}

template <int NK, bool ROWS>
__global__ __launch_bounds__(64) void rq_followers_k(FollowersArgs a)
{
    const int64_t r = blockIdx.x;
    const int NS = a.log.n_sinks;
    const Replayed p = replay<NK, ROWS, true, true, false>(a, a.log, r, 0, NS, NS);
    store_replica(a, r, p.have, p.tie, p.r2acc);
}

template <int NK, bool ROWS>
__global__ __launch_bounds__(64) void rq_followers_tile_k(FollowersTiledArgs a)
{
    const int64_t r = blockIdx.x / (unsigned)a.n_tiles;
    const int tile = (int)(blockIdx.x - r * a.n_tiles);
    const int NS = a.f.log.n_sinks;
    const int W = NS < TS ? NS : TS;                // LDS width: the launch's tile capacity
    const int x0 = tile * TS;
    const int nt = NS - x0 < TS ? NS - x0 : TS;     // this tile's columns
    LogView v = a.f.log;
    v.csr_ptr = a.tile_ptr + (size_t)tile * (v.n_str + 1);
    v.csr_col = a.tile_col;
    const Replayed p = replay<NK, ROWS, true, false, true>(a.f, v, r, x0, nt, W);
    if (lane_id() == 0) a.flags[r * a.n_tiles + tile] = p.tie ? 1 : 0;
}

__global__ __launch_bounds__(64) void rq_followers_r2_k(FollowersTiledArgs a)
{
    const int lane = lane_id();
    const int64_t r = blockIdx.x;
    const int NS = a.f.log.n_sinks;
    const Replayed p = replay<1, false, false, true, false>(a.f, a.f.log, r, 0, NS, NS);

    int fl = 0;
    for (int i = lane; i < a.n_tiles; i += 64) fl |= a.flags[r * a.n_tiles + i];
    const bool tie = __ballot((fl & 1) != 0) != 0;
    if (tie || !p.have) {
        const int64_t n = (int64_t)NS * (a.f.nK + 2);
        double* V = a.f.vals + r * n;
        for (int64_t k = lane; k < n; k += 64) V[k] = __builtin_nan("");
    }
    store_replica(a.f, r, p.have, tie, p.r2acc);
}

template <int NK>
hipError_t launch_nk(const FollowersArgs& a, hipStream_t s)
{
    const size_t lds = (size_t)a.log.n_sinks * rq_followers_sink_bytes(NK, a.rows != nullptr);
    const dim3 grid((unsigned)a.log.n_rep), block(64);
    if (a.rows) hipLaunchKernelGGL((rq_followers_k<NK, true>), grid, block, lds, s, a);
    else hipLaunchKernelGGL((rq_followers_k<NK, false>), grid, block, lds, s, a);
    return hipGetLastError();
}

template <int NK>
hipError_t launch_tiles(const FollowersTiledArgs& a, hipStream_t s)
{
    const bool rows = a.f.rows != nullptr;
    const int W = a.f.log.n_sinks < TS ? a.f.log.n_sinks : TS;
    const size_t lds = (size_t)W * rq_followers_sink_bytes(NK, rows);
    const dim3 grid((unsigned)(a.f.log.n_rep * a.n_tiles)), block(64);
    if (rows) hipLaunchKernelGGL((rq_followers_tile_k<NK, true>), grid, block, lds, s, a);
    else hipLaunchKernelGGL((rq_followers_tile_k<NK, false>), grid, block, lds, s, a);
    return hipGetLastError();
}

}  // namespace

hipError_t rq_launch_followers(const FollowersArgs& a, hipStream_t s)
{
    switch (a.nK) {
    case 1: return launch_nk<1>(a, s);
    case 2: return launch_nk<2>(a, s);
    case 3: return launch_nk<3>(a, s);
    case 4: return launch_nk<4>(a, s);
    }
    return hipErrorInvalidValue;
}

hipError_t rq_launch_followers_tiled(const FollowersTiledArgs& a, hipStream_t s)
{
    hipError_t e = hipErrorInvalidValue;
    switch (a.f.nK) {
    case 1: e = launch_tiles<1>(a, s); break;
    case 2: e = launch_tiles<2>(a, s); break;
    case 3: e = launch_tiles<3>(a, s); break;
    case 4: e = launch_tiles<4>(a, s); break;
    }
    if (e != hipSuccess) return e;
    const size_t lds = (size_t)a.f.log.n_sinks * sizeof(int);
    hipLaunchKernelGGL(rq_followers_r2_k, dim3((unsigned)a.f.log.n_rep), dim3(64), lds, s, a);
    return hipGetLastError();
}

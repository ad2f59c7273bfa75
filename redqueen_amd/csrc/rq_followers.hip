// rq_followers.hip -- per-follower metrics straight from a batch's compact event logs
// (rq_log_followers): for every sink column of rank_of_src_in_df's pivot table
// (utils.py:38-56) the integrals of I(r_i <= K-1), r_i and r_i^2 over the column's seen
// span -- the per-follower terms of the paper's objective and of utils.py:84-128 -- plus
// the sink's first-row time and its own / wall row counts, and per replica
// int_r_2_true (utils.py:124-128), the integral of the row mean of r^2.
//
// One wavefront per replica, one block per wavefront.  The wave replays the replica's
// (t, stream) log in order (log_walk, rq_log_walk.h) against per-sink state private to it
// in LDS, SoA over the graph's sink index:
//   tlast[x]   f64  time of x's last row
//   acc[q][x]  f64  the NK + 2 running integrals of x
//   rank[x]    i32  the controlled source's rank in x's feed (-1: no row yet; next_rank)
//   rows[c][x] i32  (ROWS only) own / wall rows of x
// Lanes take the event's CSR row 64 sinks per round.  A sink's rank is constant between
// two of its rows, so a row at t closes the interval [tlast, t) of the rank it replaces:
// acc_q = acc_q + f_q(rank) * (t - tlast), sequentially in time order from 0.0 and with no
// contraction -- the sum a host loop in the same order reproduces bit for bit.  A row at
// tlast itself is a duplicate (t, sink) pivot cell (RQ_ST_TIE).
//   The replica's pivot row (the state after the last event of a time) enters r2_true as
// sumR2 / nvalid: nvalid seen sinks and the exact integer sumR2 = sum of their rank^2,
// kept up to date per event with a ballot and a wave sum (a wall row adds 2 rank + 1, or 1
// for a new sink; an own row removes rank^2).  ev_cap <= 2^24 bounds rank^2 below 2^48.
//   Every output element is written exactly once by its replica's wave: first_t when the
// sink's first row plays (NaN at the end for a sink without one), everything else when the
// log has ended.  No atomics, no zeroing pass, no dependence on the launch geometry.
#include <hip/hip_runtime.h>

#include "rq_device.h"
#include "rq_internal.h"
#include "rq_log_walk.h"

#pragma clang fp contract(off)

using namespace rq;

namespace {

template <int NK, bool ROWS>
__global__ __launch_bounds__(64) void rq_followers_k(FollowersArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double lds_fl[];
    constexpr int NV = NK + 2;
    const int lane = lane_id();
    const int64_t r = blockIdx.x;
    const int NS = a.log.n_sinks;
    double* tlast = lds_fl;                                          // [NS]
    double* acc = lds_fl + NS;                                       // [NV][NS]
    int* rank = reinterpret_cast<int*>(lds_fl + (size_t)NS * (NV + 1));   // [NS]
    int* rown = rank + NS;                                           // [2][NS], ROWS only
    for (int x = lane; x < NS; x += 64) {
        tlast[x] = 0.0;
#pragma unroll
        for (int q = 0; q < NV; ++q) acc[(size_t)q * NS + x] = 0.0;
        rank[x] = -1;
        if (ROWS) {
            rown[x] = 0;
            rown[NS + x] = 0;
        }
    }
    wave_lds_sync();

    double* V = a.vals + r * NS * NV;
    double* FT = a.first_t + r * NS;
    int32_t* RW = ROWS ? a.rows + r * NS * 2 : nullptr;
    int Km1[NK];
#pragma unroll
    for (int q = 0; q < NK; ++q) Km1[q] = a.Ks[q] - 1;

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
                acc[(size_t)q * NS + x] = acc[(size_t)q * NS + x] + f * len;
            }
            acc[(size_t)NK * NS + x] = acc[(size_t)NK * NS + x] + rho * len;
            acc[(size_t)(NK + 1) * NS + x] = acc[(size_t)(NK + 1) * NS + x] + (rho * rho) * len;
        }
    };

    log_walk(a.log, r, [&](double t, bool own, int p0, int p1, int xfirst) {
        // a new time closes the pivot row that held since cur_t
        if (have && t != cur_t) r2acc = r2acc + ((double)sumR2 / (double)nvalid) * (t - cur_t);
        have = true;
        cur_t = t;
        int64_t d2 = 0;   // this lane's share of |delta sumR2|, < 2^55
        int dv = 0;
        for (int e = p0; e < p1; e += 64) {
            const bool act = e + lane < p1;
            const int x = row_sink(a.log, e, p0, act, xfirst);
            const int rk = act ? rank[x] : 0;
            if (act) {
                if (rk >= 0) {
                    const double tl = tlast[x];
                    if (tl == t) tie_l = true;
                    close_span(x, rk, tl, t);
                    d2 += own ? (int64_t)rk * rk : (int64_t)(2 * rk + 1);
                } else {
                    FT[x] = t;
                    if (!own) d2 += 1;
                }
                rank[x] = next_rank(own, rk);
                tlast[x] = t;
                if (ROWS) rown[(own ? 0 : NS) + x] = rown[(own ? 0 : NS) + x] + 1;
            }
            dv += popc(__ballot(act && rk < 0));
        }
        wave_lds_sync();
        nvalid += dv;
        const int64_t d = wave_sum_i64(d2);
        sumR2 += own ? -d : d;
    });
    // the last ranks and the last pivot row hold until end_time
    if (have) r2acc = r2acc + ((double)sumR2 / (double)nvalid) * (a.log.end - cur_t);
    for (int x = lane; x < NS; x += 64) {
        const int rk = rank[x];
        if (rk >= 0) close_span(x, rk, tlast[x], a.log.end);
    }
    wave_lds_sync();

    const bool tie = __ballot(tie_l) != 0;
    const bool bad = tie || !have;
    const double NaN = __builtin_nan("");
    for (int k = lane; k < NS * NV; k += 64) {
        const int x = k / NV, q = k - x * NV;
        V[k] = bad ? NaN : acc[(size_t)q * NS + x];
    }
    for (int x = lane; x < NS; x += 64)
        if (rank[x] < 0) FT[x] = NaN;
    if (ROWS)
        for (int k = lane; k < 2 * NS; k += 64) RW[k] = rown[(k & 1) * NS + (k >> 1)];
    if (lane == 0) {
        a.r2_true[r] = bad ? NaN : r2acc;
        a.status[r] = log_status(have, tie);
    }
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

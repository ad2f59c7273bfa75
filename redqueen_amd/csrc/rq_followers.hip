// rq_followers.hip -- per-follower metrics straight from a batch's compact event logs
// (rq_log_followers): for every sink column of rank_of_src_in_df's pivot table
// (utils.py:38-56) the integrals of I(r_i <= K-1), r_i and r_i^2 over the column's seen
// span -- the per-follower terms of the paper's objective and of utils.py:84-128 -- plus
// the sink's first-row time and its own / wall row counts, and per replica
// int_r_2_true (utils.py:124-128), the integral of the row mean of r^2.
//
// One wavefront per replica, one block per wavefront, as rq_timeline.hip.  The wave
// replays the replica's (t, stream) log in order against per-sink state private to it
// in LDS, SoA over the graph's sink index:
//   tlast[x]   f64  time of x's last row
//   acc[q][x]  f64  the NK + 2 running integrals of x
//   rank[x]    i32  the controlled source's rank in x's feed (-1: no row yet) -- the rule
//                   of rq_sweep_core.h: an own row sets 0, any other row adds 1 (unseen -> 1)
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
//
// Loads: event times, streams and CSR row bounds are fetched 64 events at a time, one
// chunk ahead; the first 64 sink columns of the next event are fetched while the
// current one is applied.
#include <hip/hip_runtime.h>

#include "rq_device.h"
#include "rq_internal.h"

#pragma clang fp contract(off)

using namespace rq;

namespace {

struct FlChunk {   // lane l: event k0 + l of the replica (an event past the log, or of a
    double t;      // stream index outside the graph, has an empty row: p0 == p1)
    int j, p0, p1;
};

template <int NK, bool ROWS>
__global__ __launch_bounds__(64) void rq_followers_k(FollowersArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double lds_fl[];
    constexpr int NV = NK + 2;
    const int lane = lane_id();
    const int64_t r = blockIdx.x;
    const int NS = a.n_sinks;
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

    int64_t n = a.counts[r * 4 + 2];
    n = n < 0 ? 0 : (n > a.ev_cap ? a.ev_cap : n);
    const double* T = a.ev_t + r * a.ev_cap;
    const int32_t* J = a.ev_src + r * a.ev_cap;
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

    auto load_chunk = [&](int64_t k0) {
        FlChunk c;
        c.t = 0.0;
        c.j = -1;
        c.p0 = c.p1 = 0;
        const int64_t k = k0 + lane;
        if (k < n) {
            c.t = T[k];
            const int j = J[k];
            if ((unsigned)j < (unsigned)a.n_str) {
                c.j = j;
                c.p0 = a.csr_ptr[j];
                c.p1 = a.csr_ptr[j + 1];
            }
        }
        return c;
    };

    FlChunk A = load_chunk(0);
    int xcur = 0;
    {
        const int q0 = bcast_i(A.p0, 0), q1 = bcast_i(A.p1, 0);
        if (q0 + lane < q1) xcur = a.csr_col[q0 + lane];
    }
    for (int64_t k0 = 0; k0 < n; k0 += 64) {
        const FlChunk B = load_chunk(k0 + 64);
        const int cnt = (int)((n - k0) < 64 ? (n - k0) : 64);
        for (int i = 0; i < cnt; ++i) {
            const double t = bcast_d(A.t, i);
            const int j = bcast_i(A.j, i);
            const int p0 = bcast_i(A.p0, i), p1 = bcast_i(A.p1, i);
            // the next event's first 64 sink columns, in flight while this one is applied
            const int q0 = i < 63 ? bcast_i(A.p0, i + 1) : bcast_i(B.p0, 0);
            const int q1 = i < 63 ? bcast_i(A.p1, i + 1) : bcast_i(B.p1, 0);
            int xnext = 0;
            if (q0 + lane < q1) xnext = a.csr_col[q0 + lane];
            if (p1 > p0) {
                // a new time closes the pivot row that held since cur_t
                if (have && t != cur_t)
                    r2acc = r2acc + ((double)sumR2 / (double)nvalid) * (t - cur_t);
                have = true;
                cur_t = t;
                const bool own = j == a.ctrl_idx;
                int64_t d2 = 0;   // this lane's share of |delta sumR2|
                int dv = 0;
                for (int e = p0; e < p1; e += 64) {
                    const bool act = e + lane < p1;
                    const int x = e == p0 ? xcur : (act ? a.csr_col[e + lane] : 0);
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
                        rank[x] = own ? 0 : (rk < 0 ? 1 : rk + 1);
                        tlast[x] = t;
                        if (ROWS) rown[(own ? 0 : NS) + x] = rown[(own ? 0 : NS) + x] + 1;
                    }
                    dv += popc(__ballot(act && rk < 0));
                }
                wave_lds_sync();
                nvalid += dv;
                // < 2^55 per lane: three 20-bit limbs keep every 64-lane sum in 32 bits
                uint32_t limb[3] = {(uint32_t)(d2 & 0xFFFFF), (uint32_t)((d2 >> 20) & 0xFFFFF),
                                    (uint32_t)(d2 >> 40)};
                wave_sum_u32_n<3>(limb);
                const int64_t l0 = (uint32_t)__builtin_amdgcn_readlane((int)limb[0], 63);
                const int64_t l1 = (uint32_t)__builtin_amdgcn_readlane((int)limb[1], 63);
                const int64_t l2 = (uint32_t)__builtin_amdgcn_readlane((int)limb[2], 63);
                const int64_t d = l0 + (l1 << 20) + (l2 << 40);
                sumR2 += own ? -d : d;
            }
            xcur = xnext;
        }
        A = B;
    }
    // the last ranks and the last pivot row hold until end_time
    if (have) r2acc = r2acc + ((double)sumR2 / (double)nvalid) * (a.end - cur_t);
    for (int x = lane; x < NS; x += 64) {
        const int rk = rank[x];
        if (rk >= 0) close_span(x, rk, tlast[x], a.end);
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
        a.status[r] = tie ? RQ_ST_TIE : (!have ? RQ_ST_EMPTY : 0);
    }
}

template <int NK>
hipError_t launch_nk(const FollowersArgs& a, hipStream_t s)
{
    const size_t lds = (size_t)a.n_sinks * rq_followers_sink_bytes(NK, a.rows != nullptr);
    const dim3 grid((unsigned)a.n_rep), block(64);
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

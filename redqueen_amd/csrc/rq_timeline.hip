// rq_timeline.hip -- time-resolved metrics straight from a batch's compact event logs
// (rq_log_timeline): the per-bin split of the integrals utils.time_in_top_k /
// average_rank / int_r_2 (utils.py:84-121) take over the pivot table of
// rank_of_src_in_df (utils.py:38-56), plus posts per bin and wall rows per (sink, bin).
//
// One wavefront per replica, one block per wavefront.  The wave replays the replica's
// (t, stream) log in order against per-sink state private to it in LDS:
//   rank[x]   the controlled source's rank in sink x's feed (-1: no row yet; next_rank);
//   grp[x]    the time group of x's last row: a second row of x in the same group is a
//             duplicate (t, sink) pivot cell (RQ_ST_TIE);
//   wcnt[x]   (wall_posts only) wall rows of x in the current bin.
// Lanes take the event's CSR row 64 sinks per round; ballots turn the per-lane changes
// into the deltas of the three integers a pivot row is made of (nvalid, sumR, c_K).
// The row holds until the next event with an edge, so the integrands are constant on
// [t_row, t_next) and the interval is clipped to the bins it meets.  Events come in
// time order: the current bin only moves forward, its sums live in registers and are
// stored once, when the bin closes -- every output element is written exactly once by
// its replica's wave, whatever n_bins (no atomics, no zeroing pass, no dependence on
// the launch geometry).  sum c_K * len is stored unnormalised; when the replica ends
// (S = its seen sinks is known) the wave divides its own values, or overwrites them
// with NaN for a TIE / EMPTY replica.
//
// The log reader and the bin clipper stand here in their own copy, the text of log_walk
// and BinClip (rq_log_walk.h): through the shared templates this kernel's one-K
// instantiation measured 3 to 4 % slower on C3.  A fix to either
// goes into both places.
#include <hip/hip_runtime.h>

#include "rq_device.h"
#include "rq_internal.h"
#include "rq_log_walk.h"

#pragma clang fp contract(off)

using namespace rq;

namespace {

template <int NK, bool WALL>
__global__ __launch_bounds__(64) void rq_timeline_k(TimelineArgs a)
{
    extern __shared__ __attribute__((aligned(16))) int lds_tl[];
    constexpr int NV = NK + 2;
    const int lane = lane_id();
    const int64_t r = blockIdx.x;
    const int NS = a.log.n_sinks;
    const int nb = a.n_bins;
    int* rank = lds_tl;
    int* grp = lds_tl + NS;
    int* wcnt = lds_tl + 2 * (size_t)NS;
    for (int x = lane; x < NS; x += 64) {
        rank[x] = -1;
        grp[x] = -1;
        if (WALL) wcnt[x] = 0;
    }
    wave_lds_sync();

    int64_t n = a.log.counts[r * 4 + 2];
    n = n < 0 ? 0 : (n > a.log.ev_cap ? a.log.ev_cap : n);
    const double* T = a.log.ev_t + r * a.log.ev_cap;
    const int32_t* J = a.log.ev_src + r * a.log.ev_cap;
    double* M = a.metrics + r * nb * NV;
    int64_t* P = a.posts + r * nb * 2;
    int32_t* W = WALL ? a.wall_posts + r * NS * (int64_t)nb : nullptr;

    // the pivot row that holds: nvalid seen sinks, sumR their ranks' sum, cK those <= K-1
    int nvalid = 0, cK[NK];
    int64_t sumR = 0;
#pragma unroll
    for (int q = 0; q < NK; ++q) cK[q] = 0;
    bool have = false, tie = false;
    double cur_t = 0.0;
    int g = 0;   // time group of cur_t
    // the open bin and its sums
    int b = 0;
    double e0 = a.edges[0], e1 = a.edges[1];
    double acc[NV];
#pragma unroll
    for (int q = 0; q < NV; ++q) acc[q] = 0.0;
    int64_t p_own = 0, p_oth = 0;

    auto close_bin = [&]() {   // store bin b, open b + 1
        if (lane == 0) {
#pragma unroll
            for (int q = 0; q < NV; ++q) M[(int64_t)b * NV + q] = acc[q];
            P[(int64_t)b * 2] = p_own;
            P[(int64_t)b * 2 + 1] = p_oth;
        }
        if (WALL) {
            for (int x = lane; x < NS; x += 64) {
                W[(int64_t)x * nb + b] = wcnt[x];
                wcnt[x] = 0;
            }
            wave_lds_sync();
        }
#pragma unroll
        for (int q = 0; q < NV; ++q) acc[q] = 0.0;
        p_own = p_oth = 0;
        ++b;
        if (b < nb) {
            e0 = a.edges[b];
            e1 = a.edges[b + 1];
        }
    };
    // the held row over [cur_t, hi), then every bin that ends at or before hi closes
    auto advance = [&](double hi) {
        double f[NV] = {};
        if (have) {
            const double m = (double)sumR / (double)nvalid;
#pragma unroll
            for (int q = 0; q < NK; ++q) f[q] = (double)cK[q];
            f[NK] = m;
            f[NK + 1] = m * m;
        }
        while (b < nb) {
            if (have) {
                const double lo = cur_t > e0 ? cur_t : e0;
                const double up = hi < e1 ? hi : e1;
                if (up > lo) {
                    const double len = up - lo;
#pragma unroll
                    for (int q = 0; q < NV; ++q) acc[q] = acc[q] + f[q] * len;
                }
            }
            if (!(e1 <= hi)) break;
            close_bin();
        }
    };

    auto load_chunk = [&](int64_t k0) {
        LogChunk c;
        c.t = 0.0;
        c.j = -1;
        c.p0 = c.p1 = 0;
        const int64_t k = k0 + lane;
        if (k < n) {
            c.t = T[k];
            const int j = J[k];
            if ((unsigned)j < (unsigned)a.log.n_str) {
                c.j = j;
                c.p0 = a.log.csr_ptr[j];
                c.p1 = a.log.csr_ptr[j + 1];
            }
        }
        return c;
    };

    LogChunk A = load_chunk(0);
    int xcur = 0;
    {
        const int q0 = bcast_i(A.p0, 0), q1 = bcast_i(A.p1, 0);
        if (q0 + lane < q1) xcur = a.log.csr_col[q0 + lane];
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
            if (q0 + lane < q1) xnext = a.log.csr_col[q0 + lane];
            if (p1 > p0) {
                advance(t);
                if (!have || t != cur_t) ++g;
                have = true;
                cur_t = t;
                const bool own = j == a.log.ctrl_idx;
                const bool inbin = b < nb && e0 <= t;   // t < e1: advance closed the bins before
                if (inbin) {
                    if (own) ++p_own;
                    else ++p_oth;
                }
                int64_t rsum = 0;   // own: this lane's share of the ranks that fall to 0
                int dv = 0, dK[NK];
#pragma unroll
                for (int q = 0; q < NK; ++q) dK[q] = 0;
                uint64_t dup = 0;
                for (int e = p0; e < p1; e += 64) {
                    const bool act = e + lane < p1;
                    const int x = e == p0 ? xcur : (act ? a.log.csr_col[e + lane] : 0);
                    const int rk = act ? rank[x] : 0;
                    const int gx = act ? grp[x] : -1;
                    const int nr = next_rank(own, rk);
                    if (act) {
                        rank[x] = nr;
                        grp[x] = g;
                        if (WALL && !own && inbin) wcnt[x] = wcnt[x] + 1;
                        if (own && rk > 0) rsum += rk;
                    }
                    dup |= __ballot(act && gx == g);
                    dv += popc(__ballot(act && rk < 0));
#pragma unroll
                    for (int q = 0; q < NK; ++q)
                        dK[q] += popc(__ballot(act && nr <= a.Ks[q] - 1)) -
                                 popc(__ballot(act && rk >= 0 && rk <= a.Ks[q] - 1));
                }
                wave_lds_sync();
                if (dup) tie = true;
                nvalid += dv;
#pragma unroll
                for (int q = 0; q < NK; ++q) cK[q] += dK[q];
                if (own) sumR -= wave_sum_i64(rsum);   // < 2^31 per sink
                else sumR += p1 - p0;
            }
            xcur = xnext;
        }
        A = B;
    }
    advance(a.log.end);   // the last row holds until end_time
    while (b < nb) close_bin();

    // S is known now: normalise the top-K sums, or blank a replica without a table.  The
    // values were stored by lane 0; the fence completes them before any lane's reload.
    const bool bad = tie || !have;
    __threadfence();
    __builtin_amdgcn_wave_barrier();
    const double NaN = __builtin_nan("");
    const double S = (double)nvalid;
    for (int64_t k = lane; k < (int64_t)nb * NV; k += 64) {
        if (bad) {
            M[k] = NaN;
        } else if ((int)(k % NV) < NK) {
            const double v = __hip_atomic_load(M + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            M[k] = v / S;
        }
    }
    if (lane == 0) a.status[r] = log_status(have, tie);
}

template <int NK>
hipError_t launch_nk(const TimelineArgs& a, hipStream_t s)
{
    const size_t lds = (size_t)a.log.n_sinks * (a.wall_posts ? 3 : 2) * sizeof(int);
    const dim3 grid((unsigned)a.log.n_rep), block(64);
    if (a.wall_posts) hipLaunchKernelGGL((rq_timeline_k<NK, true>), grid, block, lds, s, a);
    else hipLaunchKernelGGL((rq_timeline_k<NK, false>), grid, block, lds, s, a);
    return hipGetLastError();
}

}  // namespace

hipError_t rq_launch_timeline(const TimelineArgs& a, hipStream_t s)
{
    switch (a.nK) {
    case 1: return launch_nk<1>(a, s);
    case 2: return launch_nk<2>(a, s);
    case 3: return launch_nk<3>(a, s);
    case 4: return launch_nk<4>(a, s);
    }
    return hipErrorInvalidValue;
}

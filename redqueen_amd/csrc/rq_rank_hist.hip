// rq_rank_hist.hip -- the rank distribution straight from a batch's compact event logs
// (rq_log_rank_hist): per time bin and per rank value rho, the seen sink-time spent at
// rank rho in the pivot table of rank_of_src_in_df (utils.py:38-56) -- the third axis
// of that table, after time (rq_timeline.hip) and the followers (rq_followers.hip).
// utils.time_in_top_k (utils.py:84-98) is the sum of the first K cells.
//
// One wavefront per replica, one block per wavefront.  The wave replays the replica's
// (t, stream) log in order (log_walk, rq_log_walk.h) against state private to it in LDS:
//   rank[x]   the controlled source's rank in sink x's feed (-1: no row yet; next_rank);
//   grp[x]    the time group of x's last row: a second row of x in the same group is a
//             duplicate (t, sink) pivot cell (RQ_ST_TIE);
//   cnt[c]    seen sinks at rank c for c < n_ranks, at rank >= n_ranks for c = n_ranks
//             (the tail); padded with zeros to NB * 64 cells.
// Lanes take the event's CSR row 64 sinks per round.  A sink that moves from cell
// min(rk, n_ranks) to min(nr, n_ranks) is an integer update of two cells: LDS integer
// atomics, whose result does not depend on their order.  An own row sends every touched
// sink to cell 0, which gets one add of the ballots' popcount per event; a move within
// the tail touches nothing.  No f64 is ever accumulated with an atomic.
//   cnt is constant between two events with an edge and is clipped to the bins it meets
// (BinClip).  Lane l owns the cells l, l + 64, ... (NB = 1, 2 or 4 per lane: the template
// parameter, so the open bin's sums stay in registers); at each event it reads its cells
// and adds cnt * len.  A closing bin is stored 64 consecutive cells per store -- every
// output element is written exactly once by its replica's wave, whatever n_bins (no
// global atomics, no zeroing pass, no dependence on the launch geometry).  When the
// replica ends (S = its seen sinks is known) the wave divides its own values, or
// overwrites them with NaN for a TIE / EMPTY replica.
#include <hip/hip_runtime.h>

#include "rq_device.h"
#include "rq_internal.h"
#include "rq_log_walk.h"

#pragma clang fp contract(off)

using namespace rq;

namespace {

__device__ __forceinline__ void cell_add(int* p, int v)
{
    __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

template <int NB>
__global__ __launch_bounds__(64) void rq_rank_hist_k(RankHistArgs a)
{
    extern __shared__ __attribute__((aligned(16))) int lds_rh[];
    const int lane = lane_id();
    const int64_t r = blockIdx.x;
    const int NS = a.log.n_sinks;
    const int nb = a.n_bins;
    const int NR = a.n_ranks;   // cells 0..NR-1: that rank; cell NR: the tail
    const int NC = NR + 1;      // <= NB * 64
    int* rank = lds_rh;
    int* grp = lds_rh + NS;
    int* cnt = lds_rh + 2 * (size_t)NS;   // [NB * 64]
    for (int x = lane; x < NS; x += 64) {
        rank[x] = -1;
        grp[x] = -1;
    }
#pragma unroll
    for (int q = 0; q < NB; ++q) cnt[lane + 64 * q] = 0;
    wave_lds_sync();

    double* H = a.hist + r * nb * NC;

    int nvalid = 0;   // seen sinks
    int mx = -1;      // the largest rank this lane gave a sink
    bool have = false, tie = false;
    double cur_t = 0.0;
    int g = 0;   // time group of cur_t
    // the open bin and this lane's cells of it
    BinClip clip(a.edges, nb);
    double acc[NB];
#pragma unroll
    for (int q = 0; q < NB; ++q) acc[q] = 0.0;

    auto store_bin = [&](int b) {
#pragma unroll
        for (int q = 0; q < NB; ++q) {
            const int c = lane + 64 * q;
            if (c < NC) H[(int64_t)b * NC + c] = acc[q];
        }
    };
    auto held = [&](double (&f)[NB]) {   // this lane's cells of the held row
#pragma unroll
        for (int q = 0; q < NB; ++q) f[q] = have ? (double)cnt[lane + 64 * q] : 0.0;
    };

    log_walk(a.log, r, [&](double t, bool own, int p0, int p1, int xfirst) {
        double f[NB];
        held(f);   // reads cnt: the previous event ended with wave_lds_sync
        clip.advance(have, cur_t, t, f, acc, store_bin);
        if (!have || t != cur_t) ++g;
        have = true;
        cur_t = t;
        int dv = 0, to0 = 0;
        uint64_t dup = 0;
        for (int e = p0; e < p1; e += 64) {
            const bool act = e + lane < p1;
            const int x = row_sink(a.log, e, p0, act, xfirst);
            const int rk = act ? rank[x] : 0;
            const int gx = act ? grp[x] : -1;
            const int nr = next_rank(own, rk);
            if (act) {
                rank[x] = nr;
                grp[x] = g;
                mx = nr > mx ? nr : mx;
                if (own) {
                    if (rk > 0) cell_add(cnt + (rk < NR ? rk : NR), -1);
                } else if (rk < NR) {   // a move within the tail touches nothing
                    if (rk >= 0) cell_add(cnt + rk, -1);
                    cell_add(cnt + (nr < NR ? nr : NR), 1);
                }
            }
            dup |= __ballot(act && gx == g);
            dv += popc(__ballot(act && rk < 0));
            if (own) to0 += popc(__ballot(act && rk != 0));   // rk == 0 stays in cell 0
        }
        if (to0 && lane == 0) cell_add(cnt, to0);
        wave_lds_sync();
        if (dup) tie = true;
        nvalid += dv;
    });
    {
        double f[NB];
        held(f);
        clip.finish(have, cur_t, a.log.end, f, acc, store_bin);
    }

    // S is known now: normalise, or blank a replica without a table.  Every lane reloads
    // the cells it stored itself; the fence completes the stores first.
    const bool bad = tie || !have;
    __threadfence();
    __builtin_amdgcn_wave_barrier();
    const double NaN = __builtin_nan("");
    const double S = (double)nvalid;
    for (int bb = 0; bb < nb; ++bb) {
#pragma unroll
        for (int q = 0; q < NB; ++q) {
            const int c = lane + 64 * q;
            if (c < NC) {
                double* p = H + (int64_t)bb * NC + c;
                if (bad) {
                    *p = NaN;
                } else {
                    const double v = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    *p = v / S;
                }
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int m = __shfl_xor(mx, o, 64);
        mx = m > mx ? m : mx;
    }
    if (lane == 0) {
        a.status[r] = log_status(have, tie);
        a.n_seen[r] = nvalid;
        a.max_rank[r] = mx;
    }
}

template <int NB>
hipError_t launch_nb(const RankHistArgs& a, hipStream_t s)
{
    const size_t lds = ((size_t)a.log.n_sinks * 2 + NB * 64) * sizeof(int);
    const dim3 grid((unsigned)a.log.n_rep), block(64);
    hipLaunchKernelGGL((rq_rank_hist_k<NB>), grid, block, lds, s, a);
    return hipGetLastError();
}

}  // namespace

hipError_t rq_launch_rank_hist(const RankHistArgs& a, hipStream_t s)
{
    const int cells = a.n_ranks + 1;
    if (cells <= 64) return launch_nb<1>(a, s);
    if (cells <= 128) return launch_nb<2>(a, s);
    if (cells <= 256) return launch_nb<4>(a, s);
    return hipErrorInvalidValue;
}

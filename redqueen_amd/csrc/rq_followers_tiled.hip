// rq_followers_tiled.hip -- rq_log_followers' outputs for graphs whose per-sink state does
// not fit one workgroup's LDS (rq_log_followers_tiled): the sink columns are cut into tiles
// of RQ_FOLLOWERS_TILE_SINKS, and two kernels run in order on the caller's stream.
//
// (a) rq_followers_tile_k: one wavefront per (replica, tile), one block per wavefront.  It
// is rq_followers_k's body (rq_followers.hip) restricted to the tile's columns [x0, x0 + nt):
// the tile's LogView (csr_ptr = tile_ptr + tile (n_str + 1), csr_col = tile_col: a CSR of
// the edges into the tile, GraphTopo) makes log_walk replay the replica's whole log and
// hand over only the rows of the wave's own sinks -- a stream without a sink in the tile has
// an empty row there and is skipped.  LDS state SoA over the tile-local column x - x0, the
// layout of rq_followers_k at width W = min(TS, n_sinks).  A sink's sums see only that
// sink's rows, sequentially in time order from 0.0, so vals, first_t and rows have
// rq_followers_k's bits whatever the tiling; they go to their global positions of the
// rq_log_followers layout.  No r2_true work: lane 0 stores flags[r][tile], bit 0 = some sink
// of the tile got two rows at one t.
//
// (b) rq_followers_r2_k: one wavefront per replica on the graph's full CSR, rank[n_sinks]
// i32 in LDS only (40,960 sinks fill 160 KiB).  rq_followers_k's nvalid / exact integer
// sumR2 / pivot-row loop restated, so r2_true has its bits.  At the end it ORs the
// replica's flags, writes status and r2_true, and overwrites vals with NaN for a TIE / EMPTY
// replica -- the one place an element is written twice; stream order after (a) makes it
// deterministic.  first_t and rows stay valid, as in rq_log_followers.
//   No atomics, no zeroing pass, nothing read past a log's count, nothing written outside
// the replica's own output rows.
#include <hip/hip_runtime.h>

#include "rq_device.h"
#include "rq_internal.h"
#include "rq_log_walk.h"

#pragma clang fp contract(off)

using namespace rq;

namespace {

constexpr int TS = RQ_FOLLOWERS_TILE_SINKS;

template <int NK, bool ROWS>
__global__ __launch_bounds__(64) void rq_followers_tile_k(FollowersTiledArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double lds_ft[];
    constexpr int NV = NK + 2;
    const int lane = lane_id();
    const int64_t r = blockIdx.x / (unsigned)a.n_tiles;
    const int tile = (int)(blockIdx.x - r * a.n_tiles);
    const int NS = a.f.log.n_sinks;
    const int W = NS < TS ? NS : TS;                // LDS width: the launch's tile capacity
    const int x0 = tile * TS;
    const int nt = NS - x0 < TS ? NS - x0 : TS;     // this tile's columns
    double* tlast = lds_ft;                                          // [W]
    double* acc = lds_ft + W;                                        // [NV][W]
    int* rank = reinterpret_cast<int*>(lds_ft + (size_t)W * (NV + 1));   // [W]
    int* rown = rank + W;                                            // [2][W], ROWS only
    for (int x = lane; x < nt; x += 64) {
        tlast[x] = 0.0;
#pragma unroll
        for (int q = 0; q < NV; ++q) acc[(size_t)q * W + x] = 0.0;
        rank[x] = -1;
        if (ROWS) {
            rown[x] = 0;
            rown[W + x] = 0;
        }
    }
    wave_lds_sync();

    LogView v = a.f.log;
    v.csr_ptr = a.tile_ptr + (size_t)tile * (v.n_str + 1);
    v.csr_col = a.tile_col;

    double* V = a.f.vals + (r * NS + x0) * NV;      // the tile's columns of replica r
    double* FT = a.f.first_t + r * NS + x0;
    int32_t* RW = ROWS ? a.f.rows + (r * NS + x0) * 2 : nullptr;
    int Km1[NK];
#pragma unroll
    for (int q = 0; q < NK; ++q) Km1[q] = a.f.Ks[q] - 1;

    bool tie_l = false;   // this lane saw a duplicate (t, sink) cell

    // the interval [tlast[x], hi) of the rank rk >= 0 that tile-local sink x holds
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
        for (int e = p0; e < p1; e += 64) {
            // a column outside the tile cannot come from tile_col; the lane sits out if it does
            const int x = row_sink(v, e, p0, e + lane < p1, xfirst) - x0;
            const bool act = e + lane < p1 && (unsigned)x < (unsigned)nt;
            if (act) {
                const int rk = rank[x];
                if (rk >= 0) {
                    const double tl = tlast[x];
                    if (tl == t) tie_l = true;
                    close_span(x, rk, tl, t);
                } else {
                    FT[x] = t;
                }
                rank[x] = next_rank(own, rk);
                tlast[x] = t;
                if (ROWS) rown[(own ? 0 : W) + x] = rown[(own ? 0 : W) + x] + 1;
            }
        }
        wave_lds_sync();
    });
    // the last ranks hold until end_time
    for (int x = lane; x < nt; x += 64) {
        const int rk = rank[x];
        if (rk >= 0) close_span(x, rk, tlast[x], v.end);
    }
    wave_lds_sync();

    const double NaN = __builtin_nan("");
    for (int k = lane; k < nt * NV; k += 64) {
        const int x = k / NV, q = k - x * NV;
        V[k] = acc[(size_t)q * W + x];
    }
    for (int x = lane; x < nt; x += 64)
        if (rank[x] < 0) FT[x] = NaN;
    if (ROWS)
        for (int k = lane; k < 2 * nt; k += 64) RW[k] = rown[(k & 1) * W + (k >> 1)];
    const bool tie = __ballot(tie_l) != 0;
    if (lane == 0) a.flags[r * a.n_tiles + tile] = tie ? 1 : 0;
}

__global__ __launch_bounds__(64) void rq_followers_r2_k(FollowersTiledArgs a)
{
    extern __shared__ __attribute__((aligned(16))) int lds_r2[];
    const int lane = lane_id();
    const int64_t r = blockIdx.x;
    const LogView& v = a.f.log;
    const int NS = v.n_sinks;
    int* rank = lds_r2;   // [NS]
    for (int x = lane; x < NS; x += 64) rank[x] = -1;
    wave_lds_sync();

    // the pivot row that holds: nvalid seen sinks, sumR2 the sum of their squared ranks
    int nvalid = 0;
    int64_t sumR2 = 0;
    bool have = false;
    double cur_t = 0.0, r2acc = 0.0;

    log_walk(v, r, [&](double t, bool own, int p0, int p1, int xfirst) {
        // a new time closes the pivot row that held since cur_t
        if (have && t != cur_t) r2acc = r2acc + ((double)sumR2 / (double)nvalid) * (t - cur_t);
        have = true;
        cur_t = t;
        int64_t d2 = 0;   // this lane's share of |delta sumR2|, < 2^55
        int dv = 0;
        for (int e = p0; e < p1; e += 64) {
            const int x = row_sink(v, e, p0, e + lane < p1, xfirst);
            const bool act = e + lane < p1 && (unsigned)x < (unsigned)NS;
            const int rk = act ? rank[x] : 0;
            if (act) {
                if (rk >= 0) d2 += own ? (int64_t)rk * rk : (int64_t)(2 * rk + 1);
                else if (!own) d2 += 1;
                rank[x] = next_rank(own, rk);
            }
            dv += popc(__ballot(act && rk < 0));
        }
        wave_lds_sync();
        nvalid += dv;
        const int64_t d = wave_sum_i64(d2);
        sumR2 += own ? -d : d;
    });
    // the last pivot row holds until end_time
    if (have) r2acc = r2acc + ((double)sumR2 / (double)nvalid) * (v.end - cur_t);

    int fl = 0;
    for (int i = lane; i < a.n_tiles; i += 64) fl |= a.flags[r * a.n_tiles + i];
    const bool tie = __ballot((fl & 1) != 0) != 0;
    const bool bad = tie || !have;
    const double NaN = __builtin_nan("");
    if (bad) {
        const int64_t n = (int64_t)NS * (a.f.nK + 2);
        double* V = a.f.vals + r * n;
        for (int64_t k = lane; k < n; k += 64) V[k] = NaN;
    }
    if (lane == 0) {
        a.f.r2_true[r] = bad ? NaN : r2acc;
        a.f.status[r] = log_status(have, tie);
    }
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

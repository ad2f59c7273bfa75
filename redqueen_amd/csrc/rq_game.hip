// rq_game.hip -- competing RedQueen broadcasters (rq_log_game): the Opt sources of a world
// -- the players -- post against each other and against the world's exogenous event log.
//
// run_dynamic (opt_model.py:271-309) asks every dynamic source for its next time after each
// event; an Opt answers from its followers' ranks (Opt.get_next_interval, :502-544): after an
// event of stream j its intensity rises by C[c][j] = sum over j's edges into c's followers of
// sqrt(s / q), and the superposition draw is T_c = min(T_c, t + Exp(1) / C[c][j]); after its
// own post it waits (T_c = +inf).  Nothing else of the world depends on the players, so the
// exogenous sources are played first (rq_run_batch's event log) and this kernel merges the
// players into that log, one event at a time: the order of the events is the computation.
//
// One wavefront per replica, four replicas a block; lane c is the player with the c-th
// smallest src_id, so the first lane at the wave's minimal pending time is the reference's
// tie winner.  Per event: a DPP wave-min over T, the next exogenous entry from the wave's
// 64-entry window by v_readlane (lane l holds entry k0 + l with its stream's tie / edge
// word, loaded coalesced), one row of the transposed inverse table [stream][player] (LDS
// when it fits, else global memory: consecutive doubles, no bank conflicts), and -- unless no
// player's rate moved (ballot) -- one Philox call whose counter is the event's number in the
// output, so a draw depends on nothing but (seed, event number).  The output log is staged
// one entry a lane and stored 64 entries at a time.
#include <hip/hip_runtime.h>

#include "rq_device.h"
#include "rq_internal.h"

#pragma clang fp contract(off)

using namespace rq;

namespace {

constexpr int kWavesPerBlock = 4;

template <bool LDS>
__global__ __launch_bounds__(64 * kWavesPerBlock) void rq_game(GameArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double lds_inv[];
    const int lane = lane_id();
    const int P = a.P;
    if constexpr (LDS) {
        const int n = a.n_str * P;
        for (int i = (int)threadIdx.x; i < n; i += 64 * kWavesPerBlock) lds_inv[i] = a.inv[i];
        __syncthreads();
    }
    const int64_t r = (int64_t)blockIdx.x * kWavesPerBlock + (int64_t)(threadIdx.x >> 6);
    if (r >= a.n_rep) return;

    const bool pl = lane < P;
    const int my_j = pl ? a.lane_stream[lane] : -1;
    const int my_col = pl ? a.lane_col[lane] : 0;
    const uint32_t key0 = pl ? a.seeds[r * P + my_col] : 0u;
    const uint32_t key1 = kind_salt(RQ_SRC_OPT, lane == a.ctrl_lane);
    const int my_edge = pl ? (a.meta[my_j] & RQ_GAME_META_EDGE) : 0;
    double T = pl ? a.start : RQ_INF;   // the pending post
    int64_t posts = 0;

    // the exogenous log: a window of 64 entries, one a lane
    int64_t n_exo = a.counts[r * 4 + 2];
    n_exo = n_exo < 0 ? 0 : (n_exo > a.ev_cap ? a.ev_cap : n_exo);
    const double* xt_row = a.ev_t + r * a.ev_cap;
    const int32_t* xj_row = a.ev_src + r * a.ev_cap;
    int64_t k = 0, k0 = 0;
    double xt = RQ_INF;
    int xj = -1, xm = 0;
    auto load_window = [&]() {
        k0 = k;
        const int64_t i = k0 + lane;
        if (i < n_exo) {
            xt = xt_row[i];
            xj = xj_row[i];
            // a stream index outside the graph: played as a static stream without edges
            xm = (unsigned)xj < (unsigned)a.n_str ? a.meta[xj] : P;
        }
    };
    if (n_exo > 0) load_window();

    double* ot_row = a.out_t + r * a.out_cap;
    int32_t* oj_row = a.out_src + r * a.out_cap;
    double ot = 0.0;
    int oj = 0;
    int64_t e = 0, n_own = 0, n_world = 0;
    bool ovf = false;

    for (;;) {
        if (a.max_events >= 0 && e >= a.max_events) break;
        const double Tm = wave_min_f64(T);
        const bool post_due = Tm <= a.end;   // false for +inf
        bool player;
        double te = 0.0;
        int je = -1, me = 0;
        if (k < n_exo) {
            const int q = (int)(k - k0);
            te = bcast_d(xt, q);
            je = bcast_i(xj, q);
            me = bcast_i(xm, q);
            player = false;
            if (post_due && Tm <= te) {
                const int cm = __ffsll((unsigned long long)__ballot(T == Tm)) - 1;
                player = Tm < te || cm < (me & 255);
            }
        } else {
            if (!post_due) break;
            player = true;
        }
        if (e >= a.out_cap) {   // an event is due and the log is full
            ovf = true;
            break;
        }
        double t;
        int j;
        bool edge;
        if (player) {
            const int cm = __ffsll((unsigned long long)__ballot(T == Tm)) - 1;
            t = Tm;
            j = bcast_i(my_j, cm);
            edge = bcast_i(my_edge, cm) != 0;
            if (lane == cm) ++posts;
        } else {
            t = te;
            j = je;
            edge = (me & RQ_GAME_META_EDGE) != 0;
            ++k;
        }

        // the event: the poster waits, every player whose rate it raises draws
        double iv = 0.0;
        if (pl && (unsigned)j < (unsigned)a.n_str) {
            if constexpr (LDS) iv = lds_inv[j * P + lane];
            else iv = a.inv[(size_t)j * P + lane];
        }
        if (my_j == j) {
            T = RQ_INF;
            iv = 0.0;
        }
        if (__ballot(iv > 0.0)) {
            uint32_t c[4] = {(uint32_t)e, (uint32_t)((uint64_t)e >> 32), 0u, 0u};
            philox4x32_10(c, key0, key1);
            const double x = rq_std_exponential(rq_uniform53(c[0], c[1]));
            const double cand = t + x * iv;
            if (iv > 0.0 && cand < T) T = cand;
        }
        if (edge) {
            if (j == a.ctrl_idx) ++n_own;
            else ++n_world;
        }
        if (lane == (int)(e & 63)) {
            ot = t;
            oj = j;
        }
        ++e;
        if ((e & 63) == 0) {   // e <= out_cap: the 64 entries are in bounds
            ot_row[e - 64 + lane] = ot;
            oj_row[e - 64 + lane] = oj;
        }
        if (!player && k - k0 == 64 && k < n_exo) load_window();
    }
    {
        const int64_t base = e & ~(int64_t)63;
        if (base + lane < e) {
            ot_row[base + lane] = ot;
            oj_row[base + lane] = oj;
        }
    }
    if (pl) a.player_posts[r * P + my_col] = posts;
    if (lane == 0) {
        a.out_counts[r * 4 + 0] = n_own;
        a.out_counts[r * 4 + 1] = n_world;
        a.out_counts[r * 4 + 2] = e;
        a.out_counts[r * 4 + 3] = 0;
        a.status[r] = (ovf ? RQ_ST_ROWS_OVERFLOW : 0) | (n_own + n_world == 0 ? RQ_ST_EMPTY : 0);
    }
}

}  // namespace

hipError_t rq_launch_game(const GameArgs& a, hipStream_t s)
{
    const dim3 grid((unsigned)((a.n_rep + kWavesPerBlock - 1) / kWavesPerBlock)), block(64 * kWavesPerBlock);
    if (a.in_lds)
        hipLaunchKernelGGL((rq_game<true>), grid, block, rqh::game_table_bytes(a.n_str, a.P), s, a);
    else
        hipLaunchKernelGGL((rq_game<false>), grid, block, 0, s, a);
    return hipGetLastError();
}

// rq_replay_sort.hip -- the replay of dataframes whose rows are NOT in time order
// (rq_metrics_replay_unsorted): the reference's metrics take any row order
// (utils.py:38-56, its is_sorted assertion commented out at :41), ranking every sink's
// rows in DATAFRAME order and only then pivoting on the sorted unique t.  Sorting the
// rows by t first gives other numbers, so the route is built from stable sorts and
// scans that keep the dataframe order where the reference observes it.
//
// rq_rp_sort: one 1024-thread workgroup per dataframe that rq_rp_fast flagged
// RP_UNSORTED (every other workgroup leaves at once).  The primitive is a stable LSD
// radix sort of the dataframe's rows, 64-bit keys with a uint32 payload, 8 bits a
// pass: digit histogram in LDS, a tile of 1024 rows ranked by wavefront ballots (the
// lanes of a wave that share a digit, 8 ballots) and per-wave digit counts, keys and
// payloads ping-ponging in the workspace.  A pass whose digit is the same for every
// row is skipped.
//
//   counts   event ids (sign bit flipped) sorted with the own flag as the lowest digit:
//            distinct ids of the own and of the other rows are boundary counts
//            (utils.py:176, opt_runs.py:47-48), whatever the order of the ids
//   stage 1  rows sorted by sink id (sign bit flipped): segment heads number the dense
//            pivot columns and give S; one running maximum over the sorted rows gives
//            rank = pos - lastown (utils.py:43-46) -- the sort is stable, so a sink's
//            rows are in dataframe order
//   stage 2  rows sorted by t (order-preserving bits of the double, -0.0 as +0.0, so
//            both share a pivot row as under ==): t-group heads number the pivot rows
//            and give their dt
//   stage 3  the t-ordered rows sorted by dense column: a sink's rows are adjacent in
//            (t, dataframe index) order, so every row learns its sink's previous rank;
//            two neighbours of one sink in one t-group are a duplicate cell
//   prefix   in t order each row changes its pivot cell by rank - previous rank (integer
//            arithmetic, as rq_rp_fast); the running totals at the last row of a t-group
//            are the pivot row rq_rp_fast would have written (rows_dt / _sum / _valid / _cnt)
//
// A dataframe with a duplicate cell (a pivot MEAN, possibly fractional) is handed to the
// given-rank instance of rq_rp_seq (rq_replay.hip), which reads rows, columns and ranks
// in t order from the sort area.  rq_rp_scan then integrates as for any dataframe.
//
// Not evaluated: an unsorted dataframe with a NaN in t keeps RQ_EUNSORTED (the reference
// drops such rows in its pivot).
//
// HBM per row of an unsorted dataframe: RP_US_SCRATCH (40) B of sort scratch + 24 B of
// t-ordered columns (rq_api.cpp rp_sort_plan); every radix pass moves 12 B per row twice.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rq_device.h"
#include "rq_internal.h"

#pragma clang fp contract(off)

using namespace rq;

namespace {

constexpr int US_B = 1024;        // threads per workgroup = rows per tile
constexpr int US_W = US_B / 64;   // waves
constexpr uint64_t US_SIGN = 0x8000000000000000ull;

struct UsLds {
    uint32_t hist[256];           // digit histogram, then the running base of every digit
    uint32_t wcnt[US_W][256];     // per wave: rows of the digit in this tile, then their base
    int64_t tot[4][US_W];         // wave totals of the block scans
    int flag[8];                  // [0] pass skipped, [1] t decreases, [2] NaN in t, [3] duplicate cell,
                                  // [4] own events, [5] other events
};

__device__ __forceinline__ int64_t us_begin(const RpArgs& a, int64_t d) { return a.df_off ? a.df_off[d] : 0; }
__device__ __forceinline__ int64_t us_end(const RpArgs& a, int64_t d) { return a.df_off ? a.df_off[d + 1] : a.n_rows; }

// order-preserving key of a time (-0.0 and +0.0 share one) and its inverse
__device__ __forceinline__ uint64_t us_tkey(double t)
{
    if (t == 0.0) t = 0.0;
    const uint64_t b = (uint64_t)__double_as_longlong(t);
    return (b >> 63) ? ~b : (b | US_SIGN);
}
__device__ __forceinline__ double us_tval(uint64_t k)
{
    return __longlong_as_double((long long)((k & US_SIGN) ? (k ^ US_SIGN) : ~k));
}

// inclusive block scans over the 1024 threads (every thread calls; two barriers each)
__device__ __forceinline__ int us_scan_add(int v, UsLds& L, int& total)
{
    const int lane = lane_id(), w = (int)(threadIdx.x >> 6);
    const int x = (int)wave_scan_add((uint32_t)v);
    if (lane == 63) L.tot[0][w] = x;
    __syncthreads();
    int pre = 0, t = 0;
    for (int k = 0; k < US_W; ++k) {
        const int y = (int)L.tot[0][k];
        pre += k < w ? y : 0;
        t += y;
    }
    __syncthreads();
    total = t;
    return x + pre;
}
__device__ __forceinline__ int us_scan_max(int v, UsLds& L, int& total)
{
    const int lane = lane_id(), w = (int)(threadIdx.x >> 6);
    int x = v;
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(x, o, 64);
        if (lane >= o) x = x > y ? x : y;
    }
    if (lane == 63) L.tot[0][w] = x;
    __syncthreads();
    int pre = INT32_MIN, t = INT32_MIN;
    for (int k = 0; k < US_W; ++k) {
        const int y = (int)L.tot[0][k];
        if (k < w) pre = pre > y ? pre : y;
        t = t > y ? t : y;
    }
    __syncthreads();
    total = t;
    return x > pre ? x : pre;
}
// four int64 sums at once (wrap-around arithmetic: packed fields stay exact)
__device__ __forceinline__ void us_scan_add4(int64_t (&v)[4], UsLds& L, int64_t (&total)[4])
{
    const int lane = lane_id(), w = (int)(threadIdx.x >> 6);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        uint64_t x = (uint64_t)v[q];
        for (int o = 1; o < 64; o <<= 1) {
            const uint64_t y = (uint64_t)__shfl_up((long long)x, o, 64);
            if (lane >= o) x += y;
        }
        v[q] = (int64_t)x;
        if (lane == 63) L.tot[q][w] = (int64_t)x;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        uint64_t pre = 0, t = 0;
        for (int k = 0; k < US_W; ++k) {
            const uint64_t y = (uint64_t)L.tot[q][k];
            pre += k < w ? y : 0;
            t += y;
        }
        v[q] = (int64_t)((uint64_t)v[q] + pre);
        total[q] = (int64_t)t;
    }
    __syncthreads();
}

// one stable radix pass over n rows on the 8-bit digit dig(key, payload): in -> out.
// Returns false (uniformly, nothing moved) when every row has the same digit.
template <class DIG>
__device__ __forceinline__ bool us_pass(const uint64_t* kin, const uint32_t* pin, uint64_t* kout,
                                        uint32_t* pout, int n, DIG dig, UsLds& L)
{
    const int tid = (int)threadIdx.x, lane = tid & 63, w = tid >> 6;
    if (tid < 256) L.hist[tid] = 0;
    for (int k = lane; k < 256; k += 64) L.wcnt[w][k] = 0;
    if (tid == 0) L.flag[0] = 0;
    __syncthreads();
    for (int i = tid; i < n; i += US_B) atomicAdd(&L.hist[dig(kin[i], pin[i])], 1u);
    __syncthreads();
    const uint32_t h = tid < 256 ? L.hist[tid] : 0u;
    if (h == (uint32_t)n) L.flag[0] = 1;
    int total;
    const int incl = us_scan_add((int)h, L, total);   // (its barriers publish flag[0])
    if (L.flag[0]) {
        __syncthreads();   // everyone has read the flag before the next pass clears it
        return false;
    }
    if (tid < 256) L.hist[tid] = (uint32_t)incl - h;   // first output slot of the digit
    __syncthreads();
    for (int b0 = 0; b0 < n; b0 += US_B) {
        const int i = b0 + tid;
        const bool valid = i < n;
        uint64_t key = 0;
        uint32_t pay = 0;
        uint32_t d = 0;
        if (valid) {
            key = kin[i];
            pay = pin[i];
            d = dig(key, pay);
        }
        // the lanes of this wave with my digit
        uint64_t peers = __ballot(valid);
#pragma unroll
        for (int bit = 0; bit < 8; ++bit) {
            const bool one = (d >> bit) & 1u;
            const uint64_t m = __ballot(valid && one);
            peers &= one ? m : ~m;
        }
        const int before = popc(peers & ((1ull << lane) - 1ull));
        if (valid && before == 0) L.wcnt[w][d] = (uint32_t)popc(peers);
        __syncthreads();
        if (tid < 256) {   // digit tid: the waves' rows in wave order behind the rows placed so far
            uint32_t run = L.hist[tid];
            for (int k = 0; k < US_W; ++k) {
                const uint32_t x = L.wcnt[k][tid];
                L.wcnt[k][tid] = run;
                run += x;
            }
            L.hist[tid] = run;
        }
        __syncthreads();
        if (valid) {
            const uint32_t at = L.wcnt[w][d] + (uint32_t)before;
            if (at < (uint32_t)n) {   // always (the histogram counted these rows)
                kout[at] = key;
                pout[at] = pay;
            }
        }
        __syncthreads();
        for (int k = lane; k < 256; k += 64) L.wcnt[w][k] = 0;
        __syncthreads();
    }
    return true;
}

// stable sort on the key bytes [b0, b1); ks / ps: the buffers that hold the rows (on
// return the sorted ones), ko / po: the other pair
__device__ __forceinline__ void us_sort(uint64_t*& ks, uint32_t*& ps, uint64_t*& ko, uint32_t*& po, int n,
                                        int b0, int b1, UsLds& L)
{
    for (int b = b0; b < b1; ++b) {
        const int sh = 8 * b;
        if (us_pass(ks, ps, ko, po, n, [sh](uint64_t k, uint32_t) { return (uint32_t)(k >> sh) & 255u; }, L)) {
            uint64_t* tk = ks; ks = ko; ko = tk;
            uint32_t* tp = ps; ps = po; po = tp;
        }
    }
}

}  // namespace

__global__ __launch_bounds__(US_B) void rq_rp_sort(RpArgs a)
{
    __shared__ UsLds L;
    const int64_t d = blockIdx.x;
    const int tid = (int)threadIdx.x;
    RpInfo* inf = a.info + d;
    const int fl = inf->flags;
    if (fl & (RP_BADOFF | RP_EMPTYDF)) return;
    // flagged unsorted -- or given up for its width before a decreasing t was met
    if (!(fl & (RP_UNSORTED | RP_GLOBAL | RP_BIG | RP_MID))) return;
    const int64_t r0 = us_begin(a, d), r1 = us_end(a, d);
    if (r0 < 0 || r1 <= r0 || r1 > a.n_rows || r1 - r0 >= ((int64_t)1 << 31)) return;
    const int n = (int)(r1 - r0);
    const double* T = a.t + r0;
    const int64_t* SRC = a.src + r0;
    const int64_t* SNK = a.sink + r0;

    if (tid < 8) L.flag[tid] = 0;
    __syncthreads();
    {
        bool dec = false, nan = false;
        for (int i = tid; i < n; i += US_B) {
            const double ti = T[i];
            nan |= ti != ti;
            dec |= i > 0 && ti < T[i - 1];
        }
        if (dec) L.flag[1] = 1;
        if (nan) L.flag[2] = 1;
    }
    __syncthreads();
    if (!L.flag[1]) return;   // in time order: the status the replay gave it stands
    if (L.flag[2]) {          // NaN in t: not evaluated
        if (tid == 0) inf->flags = fl | RP_UNSORTED;
        return;
    }

    char* scr = a.us_scratch + (size_t)RP_US_SCRATCH * (size_t)r0;
    uint64_t* ks = reinterpret_cast<uint64_t*>(scr);
    uint64_t* ko = ks + n;
    uint32_t* ps = reinterpret_cast<uint32_t*>(ko + n);
    uint32_t* po = ps + n;
    int* colx = reinterpret_cast<int*>(po + n);   // per dataframe row: dense column, rank
    int* rankx = colx + n;
    double* Ut = a.us_t + r0;
    int* Ucol = a.us_col + r0;
    int* Urank = a.us_rank + r0;
    int* Uprev = a.us_prev + r0;
    int* Ug = a.us_g + r0;

    // ---- counts: distinct event ids of the own rows and of the others ----
    if (a.eid) {
        const int64_t* E = a.eid + r0;
        for (int i = tid; i < n; i += US_B) {
            ks[i] = (uint64_t)E[i] ^ US_SIGN;
            ps[i] = SRC[i] == a.src_id ? 1u : 0u;
        }
        __syncthreads();
        if (us_pass(ks, ps, ko, po, n, [](uint64_t, uint32_t p) { return p & 1u; }, L)) {
            uint64_t* tk = ks; ks = ko; ko = tk;
            uint32_t* tp = ps; ps = po; po = tp;
        }
        us_sort(ks, ps, ko, po, n, 0, 8, L);
        // within one id the other rows stand before the own rows
        int no = 0, nw = 0;
        for (int i = tid; i < n; i += US_B) {
            const bool head = i == 0 || ks[i] != ks[i - 1];
            const bool own = ps[i] != 0;
            no += own && (head || ps[i - 1] == 0);
            nw += !own && head;
        }
        if (no) atomicAdd(&L.flag[4], no);
        if (nw) atomicAdd(&L.flag[5], nw);
        __syncthreads();
    }

    // ---- stage 1: dense column and rank of every row, in dataframe order per sink ----
    for (int i = tid; i < n; i += US_B) {
        ks[i] = (uint64_t)SNK[i] ^ US_SIGN;
        ps[i] = (uint32_t)i;
    }
    __syncthreads();
    us_sort(ks, ps, ko, po, n, 0, 8, L);
    int S = 0;
    {
        int cmax = -1;   // the latest own row or the row before the segment's head
        for (int b0 = 0; b0 < n; b0 += US_B) {
            const int i = b0 + tid;
            const bool valid = i < n;
            bool head = false, own = false;
            uint32_t idx = 0;
            if (valid) {
                head = i == 0 || ks[i] != ks[i - 1];
                idx = ps[i] < (uint32_t)n ? ps[i] : 0u;   // (a payload is a row of the dataframe)
                own = SRC[idx] == a.src_id;
            }
            int tot, mtot;
            const int c = S + us_scan_add(head ? 1 : 0, L, tot) - 1;
            int m = us_scan_max(!valid ? -1 : own ? i : head ? i - 1 : -1, L, mtot);
            m = m > cmax ? m : cmax;
            if (valid) {
                colx[idx] = c;
                rankx[idx] = i - m;
            }
            S += tot;
            cmax = cmax > mtot ? cmax : mtot;
        }
    }
    __syncthreads();

    // ---- stage 2: pivot row of every row; rows, columns and ranks in t order ----
    for (int i = tid; i < n; i += US_B) {
        ks[i] = us_tkey(T[i]);
        ps[i] = (uint32_t)i;
    }
    __syncthreads();
    us_sort(ks, ps, ko, po, n, 0, 8, L);
    int npiv = 0;
    for (int b0 = 0; b0 < n; b0 += US_B) {
        const int i = b0 + tid;
        const bool valid = i < n;
        bool head = false;
        uint64_t key = 0;
        if (valid) {
            key = ks[i];
            head = i == 0 || key != ks[i - 1];
        }
        int tot;
        const int g = npiv + us_scan_add(head ? 1 : 0, L, tot) - 1;
        if (valid) {
            const uint32_t idx = ps[i] < (uint32_t)n ? ps[i] : 0u;
            const int c = colx[idx], r = rankx[idx];
            const double ti = us_tval(key);
            Ug[i] = g;
            Ut[i] = ti;
            Ucol[i] = c;
            Urank[i] = r;
            ko[i] = ((uint64_t)(uint32_t)c << 32) | (uint32_t)r;   // stage 3's rows
            po[i] = (uint32_t)i;
            const uint64_t kn = i + 1 < n ? ks[i + 1] : 0;
            if (i + 1 == n || kn != key) a.rows_dt[r0 + g] = (i + 1 == n ? a.end : us_tval(kn)) - ti;
        }
        npiv += tot;
    }
    __syncthreads();

    // ---- stage 3: a sink's rows adjacent in (t, dataframe index) order ----
    {
        uint64_t* tk = ks; ks = ko; ko = tk;
        uint32_t* tp = ps; ps = po; po = tp;
    }
    us_sort(ks, ps, ko, po, n, 4, 8, L);   // on the column alone: the sort is stable
    {
        bool dup = false;
        for (int i = tid; i < n; i += US_B) {
            const uint64_t key = ks[i];
            const uint32_t p = ps[i] < (uint32_t)n ? ps[i] : 0u;
            int prev = -1;
            if (i > 0 && (ks[i - 1] >> 32) == (key >> 32)) {
                const uint32_t pp = ps[i - 1] < (uint32_t)n ? ps[i - 1] : 0u;
                prev = (int)(uint32_t)ks[i - 1];
                dup |= Ug[pp] == Ug[p];
            }
            Uprev[p] = prev;
        }
        if (dup) L.flag[3] = 1;
    }
    __syncthreads();
    const bool dup = L.flag[3] != 0;

    if (tid == 0) {
        inf->S = S;
        inf->n_piv = npiv;   // (a duplicate cell: rq_rp_seq counts them again)
        inf->n_own = L.flag[4];
        inf->n_world = L.flag[5];
        inf->flags = RP_SORTED | (dup ? RP_FALLBACK : 0);
    }
    if (dup) return;

    // ---- the pivot rows: running totals of the cells' changes in t order ----
    const int nK = a.nK;
    int64_t carry[4] = {0, 0, 0, 0};   // cell sum; #valid | #<=K0-1 << 32; K1 | K2 << 32; K3
    for (int b0 = 0; b0 < n; b0 += US_B) {
        const int i = b0 + tid;
        const bool valid = i < n;
        int64_t v[4] = {0, 0, 0, 0}, tot[4];
        int g = 0, gn = -1;
        if (valid) {
            const int rank = Urank[i], prev = Uprev[i];
            g = Ug[i];
            gn = i + 1 < n ? Ug[i + 1] : -1;
            const bool pnan = prev < 0;
            int c[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int km1 = a.Ks[q] - 1;
                c[q] = q < nK ? (rank <= km1 ? 1 : 0) - ((!pnan && prev <= km1) ? 1 : 0) : 0;
            }
            v[0] = (int64_t)rank - (pnan ? 0 : prev);
            v[1] = (int64_t)(pnan ? 1 : 0) + (int64_t)((uint64_t)(int64_t)c[0] << 32);
            v[2] = (int64_t)c[1] + (int64_t)((uint64_t)(int64_t)c[2] << 32);
            v[3] = c[3];
        }
        us_scan_add4(v, L, tot);
        if (valid && gn != g) {
            const uint64_t x1 = (uint64_t)(carry[1] + v[1]), x2 = (uint64_t)(carry[2] + v[2]);
            const uint32_t cq[4] = {(uint32_t)(x1 >> 32), (uint32_t)x2, (uint32_t)(x2 >> 32),
                                    (uint32_t)(carry[3] + v[3])};
            const int64_t row = r0 + g;
            a.rows_sum[row] = (double)(carry[0] + v[0]);
            a.rows_valid[row] = (uint32_t)x1;
            for (int q = 0; q < nK; ++q) a.rows_cnt[row * nK + q] = cq[q];
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) carry[q] = (int64_t)((uint64_t)carry[q] + (uint64_t)tot[q]);
    }
}

hipError_t rq_launch_rp_sort(const RpArgs& a, hipStream_t s)
{
    if (a.n_df <= 0 || !a.us_scratch) return hipSuccess;
    hipLaunchKernelGGL(rq_rp_sort, dim3((unsigned)a.n_df), dim3(US_B), 0, s, a);
    return hipGetLastError();
}

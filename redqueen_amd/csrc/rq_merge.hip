// rq_merge.hip -- the general fast sweep's arrival merge as its own kernel.
//
// Manager.run_dynamic (opt_model.py:241-314) plays the other sources' events in
// (time, source) order; with > 64 sources the arrivals are pre-generated per source
// (rq_gen_streams), and a sweep wave that merges 500 streams itself touches each
// source's stream 8 bytes at a time -- the lines are evicted between touches (round 2:
// ~10x the algorithmic read bytes).  Here one block per replica merges them once:
//
//   thread j owns source j (<= RQ_MG_B sources; a one-wave block for <= 64) and reads
//   its stream in aligned
//   64-byte chunks (two in registers, the next load issued between rounds), so every
//   line is read once;
//   rounds: every arrival before a cut tau (tau adapts so a round holds ~MG_TARGET)
//   goes to an LDS buffer with its time sub-bucket (M equal slices of [t_lo, tau),
//   a monotone map of t) and its slot in that bucket (LDS atomics), a block scan of the
//   bucket counts places the buckets, and each arrival's rank inside its bucket --
//   (t, source, buffer index) order, a bucket holds ~1 arrival -- gives its place;
//   the round is written out contiguously: mrg_t f64 / mrg_j u16 [replica][capsum].
//
// A source's arrivals enter the buffer in stream order (a lane's buffer indices grow),
// so equal times keep stream order within a source and source order across sources:
// the order the windowed sweep's stage rank gives (rq_device.h stage_rank).
// More than MG_CAP arrivals at ONE time (only replayed data can do that) cannot be
// ordered in a round: the block emits them MG_CAP at a time and flags RQ_ST_TIE, which
// sends the batch to the exact sequential sweep (engine.Graph.run(check=True)).
//
// 9-64 streams in one level go to rq_merge_flat below (the same output from windows in
// which a lane holds an arrival, not a stream); <= 8 to the ranking merge rq_merge_rank.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cstdlib>
#include <type_traits>

#include "rq_device.h"
#include "rq_internal.h"

#pragma clang fp contract(off)

using namespace rq;

namespace {

// block sizes: RQ_MG_B (512) threads for 65-512 sources, one wave for <= 64 (the fused
// sweep's worlds); per block size B: rounds of <= 4B arrivals over 4B sub-buckets
constexpr int MG_SB = 11;           // bits of a slot / buffer index (< MG_CAP)
template <int B>
struct MgCfg {
    static constexpr int W = B / 64;
    static constexpr int CAP = 4 * B;       // arrivals per round (LDS buffer)
    static constexpr int M = 4 * B;         // time sub-buckets per round (4 per thread in the scan)
    static constexpr int TARGET = 3 * B;    // arrivals a round aims at
    static_assert(CAP <= (1 << MG_SB) && M <= (1 << MG_SB), "packed fields");
};

// eight consecutive arrivals of one stream (a 64-byte aligned chunk)
struct Chunk {
    double4 a, b;
};

__device__ __forceinline__ double sel8(Chunk c, int k)
{
    const double a0 = (k & 1) ? c.a.y : c.a.x, a1 = (k & 1) ? c.a.w : c.a.z;
    const double a2 = (k & 1) ? c.b.y : c.b.x, a3 = (k & 1) ? c.b.w : c.b.z;
    const double b0 = (k & 2) ? a1 : a0, b1 = (k & 2) ? a3 : a2;
    return (k & 4) ? b1 : b0;
}

__device__ __forceinline__ Chunk load_chunk(const double* p)
{
    const double4* q = reinterpret_cast<const double4*>(p);
    return Chunk{q[0], q[1]};
}

// the second half of a 128-byte line, whose first half was read before: nothing reads
// the line again, so it is loaded non-temporally (the L2 may drop it first and keep the
// lines whose second half is still to come)
typedef double rq_v4d __attribute__((ext_vector_type(4)));
__device__ __forceinline__ Chunk load_chunk_last(const double* p)
{
    const rq_v4d* q = reinterpret_cast<const rq_v4d*>(p);
    const rq_v4d x = __builtin_nontemporal_load(q), y = __builtin_nontemporal_load(q + 1);
    return Chunk{make_double4(x.x, x.y, x.z, x.w), make_double4(y.x, y.y, y.z, y.w)};
}

// arrival k (0..15) of the two chunks; both halves selected as values (a select of the
// chunks themselves would put them in scratch memory)
__device__ __forceinline__ double sel16(Chunk c, Chunk nx, int k)
{
    const double x0 = sel8(c, k & 7), x1 = sel8(nx, k & 7);
    return (k & 8) ? x1 : x0;
}

// sub-bucket of t in [t_lo, tau): non-decreasing in t (a NaN scale -- tau one ulp
// above t_lo = 0 -- sends every arrival of the round to the last bucket)
template <int M>
__device__ __forceinline__ int sub_of(double t, double t_lo, double scale)
{
    const double x = (t - t_lo) * scale;
    return x < (double)(M - 1) ? (int)x : M - 1;
}

}  // namespace

// the u16 stream of arrival k (0..15) of two 8-entry chunks of a sub-merge input
__device__ __forceinline__ uint32_t selj16(uint4 c, uint4 nx, int k)
{
    const uint4 v = (k & 8) ? nx : c;
    const uint32_t w0 = (k & 2) ? v.y : v.x, w1 = (k & 2) ? v.w : v.z;
    const uint32_t w = (k & 4) ? w1 : w0;
    return (k & 1) ? (w >> 16) : (w & 0xFFFFu);
}

// SUB: the second level of a two-level merge (> RQ_MG_B sources): thread g owns the
// merged sequence of stream group g (its entries carry their own stream ids)
// WIDE: more than 65535 streams (the second level writes bits 16-23 to out_jh)
template <int MG_B, bool SUB, bool WIDE = false>
__global__ __launch_bounds__(MG_B) void rq_merge_streams(MergeArgs a)
{
    constexpr int MG_W = MgCfg<MG_B>::W, MG_CAP = MgCfg<MG_B>::CAP, MG_M = MgCfg<MG_B>::M;
    constexpr int MG_TARGET = MgCfg<MG_B>::TARGET;
    // the one-wave instance (<= 64 streams, rounds of <= 256) keeps its slot / sub-bucket
    // pair, stream and bucket bases in 16 bits: 7.7 instead of 9.2 KB per block, so 20
    // blocks share a CU (its VGPR bound) instead of 17
    constexpr bool NARROW = MG_B <= 64 && !SUB;
    constexpr int BS_SH = NARROW ? 8 : MG_SB;   // bs = (sub-bucket << BS_SH) | slot
    static_assert(!NARROW || (MG_CAP <= 256 && MG_M <= 256), "16-bit fields");
    using BS_T = typename std::conditional<NARROW, uint16_t, uint32_t>::type;
    using BJ_T = typename std::conditional<WIDE, uint32_t, uint16_t>::type;   // global ids > 65535
    __shared__ double bt[MG_CAP];          // round buffer (arrival order)
    __shared__ BS_T bs[MG_CAP];            // (sub-bucket << BS_SH) | slot
    __shared__ BJ_T bj[MG_CAP];            // the arrival's stream
    __shared__ double st[MG_CAP];          // bucket order
    __shared__ uint32_t sk[MG_CAP];        // (stream << MG_SB) | buffer index (streams < 2^21)
    __shared__ uint32_t cnt[MG_M];
    __shared__ BS_T bbase[MG_M + 1];
    __shared__ double wmin[MG_W];
    __shared__ uint32_t wsum[MG_W];
    __shared__ uint32_t nb;

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int64_t rl = blockIdx.x;
    // the first level of a two-level merge: block (rl, group) merges streams
    // [group MG_B, group MG_B + MG_B); one level: gridDim.y == 1
    const int grp = SUB ? 0 : (int)blockIdx.y, ngrp = SUB ? 1 : (int)gridDim.y;
    const int j = (SUB ? 0 : grp * MG_B) + tid;
    // the stream id an entry carries out: group-local at a two-level merge's first level
    // (< RQ_MG_B: u16 whatever the source count), global otherwise; the second level
    // (SUB) turns its group g's local ids back into global ones, g RQ_MG_B + local
    const uint32_t jout = SUB ? (uint32_t)tid * (uint32_t)a.grp_sz : (uint32_t)(j - grp * MG_B);
    int L = 0;
    const double* src = a.streams;
    const uint16_t* srcj = nullptr;   // SUB: the entries' own stream ids
    if constexpr (SUB) {
        srcj = a.sub_j;
        src = a.sub_t;
        if (tid < a.n_grp) {
            const int64_t q = rl * a.n_grp + tid;
            L = a.sub_len[q];
            src = a.sub_t + q * a.sub_stride;
            srcj = a.sub_j + q * a.sub_stride;
        }
    } else if (j < a.n_str) {
        L = a.slen[(int64_t)j * a.slen_stride + rl];
        src = a.streams + rl * a.capsum + a.st_off[j];
    }
    // the stream's aligned chunks [p8, p8 + 8) in c and [p8 + 8, p8 + 16) in nx, with
    // p8 <= p < p8 + 16: a round's walk reads registers only; after the walk a lane that
    // moved into nx shifts it down and issues the load of the next chunk, which has the
    // rest of the round to arrive (a lane that runs through both chunks inside one walk
    // -- a burst -- loads synchronously)
    // (loads are unconditional, clamped to the stream's last chunk -- or to the buffer's
    // start for an empty stream -- so they land straight in c / nx and are waited for
    // only where the values are used)
    Chunk c, nx;
    uint4 cj = make_uint4(0, 0, 0, 0), nxj = make_uint4(0, 0, 0, 0);   // SUB: the chunks' stream ids
    int p = 0, p8 = 0;
    const int lastc = L > 0 ? (L - 1) & ~7 : 0;
#define RQ_MG_CHUNK(q) load_chunk(src + ((q) < lastc ? (q) : lastc))
#define RQ_MG_JCHUNK(q) (*reinterpret_cast<const uint4*>(srcj + ((q) < lastc ? (q) : lastc)))
#define RQ_MG_RELOAD(p0)                 \
    do {                                 \
        p8 = (p0) & ~7;                  \
        c = RQ_MG_CHUNK(p8);             \
        nx = RQ_MG_CHUNK(p8 + 8);        \
        if (SUB) {                       \
            cj = RQ_MG_JCHUNK(p8);       \
            nxj = RQ_MG_JCHUNK(p8 + 8);  \
        }                                \
    } while (0)
#define RQ_MG_HEAD() (p < L ? sel16(c, nx, p - p8) : RQ_INF)
    RQ_MG_RELOAD(0);
    double head = L > 0 ? c.a.x : RQ_INF;

    for (int k = tid; k < MG_M; k += MG_B) cnt[k] = 0;
    if (tid == 0) nb = 0;
    {
        const double m = wave_min_f64(head);
        const uint32_t s = wave_sum_u32((uint32_t)L);
        if (lane == 0) {
            wmin[w] = m;
            wsum[w] = s;
        }
    }
    __syncthreads();
    double t_lo = wmin[0];
    uint32_t total = 0;
#pragma unroll
    for (int k = 0; k < MG_W; ++k) {
        t_lo = wmin[k] < t_lo ? wmin[k] : t_lo;
        total += wsum[k];
    }
    double span = (a.end - t_lo) * ((double)MG_TARGET / (double)(total > 1 ? total : 1));
    int64_t outpos = 0;
    double* out_t = a.out_t + (rl * ngrp + grp) * a.mrg_stride;
    uint16_t* out_j = a.out_j + (rl * ngrp + grp) * a.mrg_stride;
    int status = 0;
    __syncthreads();   // wmin / wsum read before the first round rewrites them
#ifdef RQ_PHASE_CLOCK
    // diagnostic builds: block-0-thread view of where a round's time goes
    unsigned long long ck[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tc0 = 0, tc1 = 0;
#define RQ_MG_TICK(k)                                                    \
    do {                                                                 \
        tc1 = __builtin_amdgcn_s_memtime();                              \
        ck[k] += tc1 - tc0;                                              \
        tc0 = tc1;                                                       \
    } while (0)
#else
#define RQ_MG_TICK(k) do { } while (0)
#endif

    while (t_lo <= a.end) {
#ifdef RQ_PHASE_CLOCK
        tc0 = __builtin_amdgcn_s_memtime();
        ck[4] += 1;
#endif
        double tau = t_lo + span;
        if (!(tau > t_lo)) tau = next_up(t_lo);
        const double scale = (double)MG_M / (tau - t_lo);
        const int p0 = p, p8_0 = p8;
        // ---- every arrival before tau into the buffer (a lane stops at a full buffer) ----
        bool more = true;
        uint32_t nb1 = 0;   // one-wave blocks: the buffer cursor
#ifndef RQ_MG_VEC
#define RQ_MG_VEC 1
#endif
        if (RQ_MG_VEC) {
            // the cached ones, every lane at once: a lane's arrivals before tau are the run
            // [k0, k0 + cl) of its 16 cached (the stream is sorted), one wave prefix sum
            // places them, and the 16 register slots are unrolled (static indices)
            const double cv[16] = {c.a.x, c.a.y, c.a.z, c.a.w, c.b.x, c.b.y, c.b.z, c.b.w,
                                   nx.a.x, nx.a.y, nx.a.z, nx.a.w, nx.b.x, nx.b.y, nx.b.z, nx.b.w};
            const int k0 = p - p8;
            int cl = 0;
#pragma unroll
            for (int k = 0; k < 16; ++k) cl += (k >= k0 && p8 + k < L && cv[k] < tau) ? 1 : 0;
            const uint32_t incl = wave_scan_add((uint32_t)cl);
            const uint32_t tot = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
            uint32_t b0;
            if constexpr (MG_W == 1) {
                b0 = nb1;
                nb1 += tot;
            } else {
                b0 = 0;
                if (lane == 0 && tot) b0 = atomicAdd(&nb, tot);
                b0 = (uint32_t)__builtin_amdgcn_readlane((int)b0, 0);
            }
            const int base = (int)(b0 + incl) - cl;
            const int room = MG_CAP - base;
            const int take = cl < room ? cl : (room > 0 ? room : 0);
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const int e = k - k0;
                if (e >= 0 && e < take) {
                    const int idx = base + e;
                    const int sb = sub_of<MG_M>(cv[k], t_lo, scale);
                    const uint32_t slot = atomicAdd(&cnt[sb], 1u);
                    bt[idx] = cv[k];
                    bj[idx] = SUB ? jout + selj16(cj, nxj, k) : jout;
                    bs[idx] = (BS_T)(((uint32_t)sb << BS_SH) | slot);
                }
            }
            p += take;
            if (take < cl) more = false;   // the buffer is full
            if (p - p8 == 16 && p < L) RQ_MG_RELOAD(p);   // a burst: both chunks consumed
            head = RQ_MG_HEAD();
        }
        // the rest of a burst (a lane ran through both chunks), one arrival per step
        for (;;) {
            const bool act = more && head < tau;
            const uint64_t m = __ballot(act);
            if (!m) break;
            uint32_t b0;
            if constexpr (MG_W == 1) {   // one wave: the buffer cursor is a register
                b0 = nb1;
                nb1 += (uint32_t)__popcll(m);
            } else {
                const int fl = __ffsll((unsigned long long)m) - 1;
                b0 = 0;
                if (lane == fl) b0 = atomicAdd(&nb, (uint32_t)__popcll(m));
                b0 = (uint32_t)__builtin_amdgcn_readlane((int)b0, fl);
            }
            if (act) {
                const uint32_t idx = b0 + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
                if (idx < (uint32_t)MG_CAP) {
                    const int sb = sub_of<MG_M>(head, t_lo, scale);
                    const uint32_t slot = atomicAdd(&cnt[sb], 1u);
                    bt[idx] = head;
                    bj[idx] = SUB ? jout + selj16(cj, nxj, p - p8) : jout;
                    bs[idx] = (BS_T)(((uint32_t)sb << BS_SH) | slot);
                    ++p;
                    if (p - p8 == 16 && p < L) RQ_MG_RELOAD(p);   // a burst: both chunks consumed
                    head = RQ_MG_HEAD();
                } else {
                    more = false;
                }
            }
        }
        {
            const double m = wave_min_f64(head);
            if (lane == 0) wmin[w] = m;
        }
        if (p - p8 >= 8) {   // into nx: its successor's load overlaps the rest of the round
            c = nx;
            p8 += 8;
#ifndef RQ_MG_NTL
#define RQ_MG_NTL 1
#endif
            if (RQ_MG_NTL && ((p8 + 8) & 8))   // the second half of its line: the line's last use
                nx = load_chunk_last(src + ((p8 + 8) < lastc ? (p8 + 8) : lastc));
            else
                nx = RQ_MG_CHUNK(p8 + 8);
            if (SUB) {
                cj = nxj;
                nxj = RQ_MG_JCHUNK(p8 + 8);
            }
        }
        if constexpr (MG_W == 1) {
            if (lane == 0) nb = nb1;
        }
        RQ_MG_TICK(0);
        __syncthreads();
        RQ_MG_TICK(1);
        const uint32_t nr_all = nb;
        uint32_t nr = nr_all;
        if (nr_all > (uint32_t)MG_CAP) {
            if (tau != next_up(t_lo)) {
                // too many for one round: undo it and halve the cut
                p = p0;   // the chunks in registers still hold p0 unless a burst or the shift moved them
                if (p8 != p8_0) RQ_MG_RELOAD(p0);
                head = RQ_MG_HEAD();
                for (int k = tid; k < MG_M; k += MG_B) cnt[k] = 0;
                __syncthreads();
                if (tid == 0) nb = 0;
                span = (tau - t_lo) * 0.5;
                __syncthreads();
#ifdef RQ_PHASE_CLOCK
                ck[5] += 1;
#endif
                continue;
            }
            // more than MG_CAP arrivals at t_lo itself: take the first MG_CAP (any subset
            // of equal times is a time prefix) and flag the replica
            nr = MG_CAP;
            status |= a.strict_ties ? RQ_ST_UNORDERED : RQ_ST_TIE;
        }
        if (outpos + (int64_t)nr > a.mrg_stride) {   // past the merged capacity (uniform)
            status |= RQ_ST_STREAM_OVERFLOW;
            break;
        }
        double t_next = wmin[0];
#pragma unroll
        for (int k = 1; k < MG_W; ++k) t_next = wmin[k] < t_next ? wmin[k] : t_next;
        // ---- bucket bases: exclusive scan of cnt (4 buckets per thread) ----
        uint32_t v0 = cnt[4 * tid], v1 = cnt[4 * tid + 1], v2 = cnt[4 * tid + 2], v3 = cnt[4 * tid + 3];
        const uint32_t tsum = v0 + v1 + v2 + v3;
        const uint32_t incl = wave_scan_add(tsum);
        if (lane == 63) wsum[w] = incl;
        __syncthreads();
        if (tid == 0) nb = 0;   // every thread read nb before this barrier
        uint32_t wo = 0;
#pragma unroll
        for (int k = 0; k < MG_W; ++k) wo += k < w ? wsum[k] : 0u;
        {
            const uint32_t b = wo + incl - tsum;
            bbase[4 * tid] = (BS_T)b;
            bbase[4 * tid + 1] = (BS_T)(b + v0);
            bbase[4 * tid + 2] = (BS_T)(b + v0 + v1);
            bbase[4 * tid + 3] = (BS_T)(b + v0 + v1 + v2);
            cnt[4 * tid] = cnt[4 * tid + 1] = cnt[4 * tid + 2] = cnt[4 * tid + 3] = 0;
            if (tid == 0) bbase[MG_M] = (BS_T)nr;
        }
        __syncthreads();
        RQ_MG_TICK(2);
        // ---- into bucket order ----
        for (int i = tid; i < (int)nr; i += MG_B) {
            const uint32_t x = bs[i];
            const uint32_t pos = (uint32_t)bbase[x >> BS_SH] + (x & ((1u << BS_SH) - 1u));
            st[pos] = bt[i];
            sk[pos] = ((uint32_t)bj[i] << MG_SB) | (uint32_t)i;
        }
        __syncthreads();
        RQ_MG_TICK(3);
        // ---- rank inside the bucket, written out in play order ----
        for (int i = tid; i < (int)nr; i += MG_B) {
            const double x = st[i];
            const uint32_t kx = sk[i];
            const int sb = sub_of<MG_M>(x, t_lo, scale);
            const int g0 = (int)bbase[sb], g1 = (int)bbase[sb + 1];
            int r = 0;
            for (int k = g0; k < g1; ++k) {
                const double y = st[k];
                r += (y < x || (y == x && sk[k] < kx)) ? 1 : 0;
            }
#ifndef RQ_MG_NT
#define RQ_MG_NT 1
#endif
            // streaming stores: the output must not evict the input lines (C3 merge reads
            // 1.71 -> 1.37 x its 8 B per arrival, profiles/r04_merge_traffic.txt)
            if (RQ_MG_NT) {
                __builtin_nontemporal_store(x, &out_t[outpos + g0 + r]);
                __builtin_nontemporal_store((uint16_t)(kx >> MG_SB), &out_j[outpos + g0 + r]);
            } else {
                out_t[outpos + g0 + r] = x;
                out_j[outpos + g0 + r] = (uint16_t)(kx >> MG_SB);
            }
            if (WIDE) a.out_jh[(rl * ngrp + grp) * a.mrg_stride + outpos + g0 + r] = (uint8_t)(kx >> (MG_SB + 16));
        }
        RQ_MG_TICK(6);
        outpos += nr;
        // next cut: aim at MG_TARGET arrivals, grow at most 4x per round
        const double wdt = tau - t_lo;
        const double f = (double)MG_TARGET / (double)(nr > 64 ? nr : 64);
        span = wdt * (f < 4.0 ? f : 4.0);
        t_lo = t_next;   // the heads after the walk (an equal-time round: t_lo again)
    }
#ifdef RQ_PHASE_CLOCK
    // phases: 0 walk, 1 barrier after the walk, 2 bucket scan, 3 scatter, 6 rank + write;
    // 4 rounds, 5 retried rounds
    if (a.clk && w == 0 && lane == 0)
        for (int k = 0; k < 8; ++k) atomicAdd(&a.clk[k], ck[k]);
#endif
#undef RQ_MG_TICK
#undef RQ_MG_HEAD
#undef RQ_MG_RELOAD
#undef RQ_MG_CHUNK
    if (tid == 0) {
        a.out_len[rl * ngrp + grp] = (int)outpos;
        if (status) atomicOr(&a.status[a.chunk0 + rl], status);
    }
}

// ---------------------------------------------------------------------------
// <= 64 streams in flat windows: the bucket rounds above give a lane a
// stream, so a round's walk runs over (stream, cache slot) pairs that are mostly empty.
// Here a block of FB threads merges a replica in windows of <= FCAP arrivals (two waves and
// 1024 as launched: the smallest step of the shapes measured), and in every
// pass over arrivals a lane slot holds an arrival:
//
//   run search: a stream is sorted, so its arrivals before the cut tau are a prefix of
//   what is left of it.  FB / 64 lanes per stream find the prefix's end by comparison
//   (an (FB / 64 + 1)-ary search from the cursor, one load per lane and step), so the
//   window's total is known before LDS is touched: a window over FCAP is retried with
//   half the span at the cost of the search alone;
//   items: an exclusive scan of the run lengths numbers the window's arrivals
//   0 .. nr - 1 in (stream, position) order; thread i, i + FB, ... finds its item's stream
//   in the 64 prefix sums (6 LDS steps), loads its time (consecutive items of a run are
//   consecutive addresses) and keeps time and key in registers across
//   (a) the histogram of time sub-buckets, (b) the in-place scan of the counts and
//   (c) the scatter into bucket order, where the bases serve as cursors and end as the
//   buckets' ends; (d) ranks every entry inside its bucket by (t, stream, position) and
//   writes it out, as the bucket rounds do.
//
// The output is the bucket rounds' element for element: every window emits all arrivals
// before its cut in (t, stream, position in stream) order, whatever the cuts are.  More
// than FCAP arrivals at ONE time are emitted FCAP at a time in (stream, position) order
// and flagged, as there with MG_CAP.
// ---------------------------------------------------------------------------
#ifndef RQ_FLAT_BT
#define RQ_FLAT_BT 7   // pre-pass chunks in flight per lane: 56 arrivals of a stream (two lanes) per round trip
#endif
#ifndef RQ_FLAT_NB
#define RQ_FLAT_NB 16   // slices of the table (16 / 32 / 64 measured)
#endif

// sub_of, kept inside the counts whatever the input (an unsorted stream's t < t_lo)
template <int M>
__device__ __forceinline__ int flat_sub(double t, double t_lo, double scale)
{
    const int sb = sub_of<M>(t, t_lo, scale);
    return sb > 0 ? sb : 0;
}

// the neighbour lane's value (lanes 2 i and 2 i + 1 swap: quad_perm [1,0,3,2])
__device__ __forceinline__ uint32_t flat_swap1(uint32_t v)
{
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, false);
}
__device__ __forceinline__ double flat_swap1_f64(double x)
{
    const uint64_t b = (uint64_t)__double_as_longlong(x);
    return __longlong_as_double((long long)(((uint64_t)flat_swap1((uint32_t)(b >> 32)) << 32) | flat_swap1((uint32_t)b)));
}

// NB > 0: windows from a slice table.  A pre-pass reads every stream once, front
// to back, with loads whose addresses depend on st_off / slen alone, and counts per stream s
// and slice b of NB equal slices of [t_min, end] the arrivals before slice b (cum, packed
// 16-bit in the registers of the stream's two lanes) and their totals over the streams (tot,
// LDS).  A window is then the longest run of whole slices from the current one that holds
// <= FCAP arrivals: its runs are cum differences, so no load decides where a run ends.
// An arrival's slice is min(NB - 1, (int)((t - t_min) * (NB / (end - t_min)))), computed in
// the pre-pass alone: the map is non-decreasing in t (equal times share a slice), so whole
// slices are time cuts whatever the rounding, and nothing tests membership again.  A replica
// with more arrivals than the merged capacity (RQ_ST_STREAM_OVERFLOW: decided before the
// pre-pass, so out_len and the emitted prefix are the search loop's), with
// a slice over FCAP (equal times among them), an inversion, a time outside [t_min, end] (NaN
// too) or a stream past the 16-bit counts takes the search loop below for the whole replica
// (block-uniform), which alone carries the one-ulp window, the NaN scale, the FCAP-at-a-time
// emission and `while (t_lo <= end)`.  NB = 0: the search loop only (RQ_FLAT_SLICES=0).
template <int FB, int FCAP, int FT8, int NB = 0>
__global__ __launch_bounds__(FB) void rq_merge_flat(MergeArgs a)
{
    constexpr int FW = FB / 64;            // waves
    constexpr int LPS = FB / 64;           // lanes per stream in the run search
    constexpr int PT = FCAP / FB;          // items (and sub-buckets) per thread
    constexpr int FM = FCAP;               // time sub-buckets per window
    constexpr int FTARGET = FT8 * FCAP / 8;   // arrivals a window aims at
    constexpr int KB = FCAP <= 1024 ? 10 : FCAP <= 2048 ? 11 : 12;   // bits of a position in a run
    constexpr int SB_SH = KB + 6;          // kv = (sub-bucket << SB_SH) | (stream << KB) | position
    static_assert(FCAP % FB == 0 && FCAP <= (1 << KB) && PT % 4 == 0 && SB_SH + KB <= 32, "packed fields");
    __shared__ double st[FCAP];            // bucket order
    __shared__ uint32_t sk[FCAP];          // (stream << KB) | position in the window's run
    __shared__ __attribute__((aligned(16))) uint32_t cnt[FM];   // counts, then bases / cursors, then ends
    __shared__ uint32_t pre[64];           // items before stream s in the window
    __shared__ uint32_t sbase[64];         // stream s's cursor as an index into the replica's streams
    __shared__ uint32_t wsum[2][FW], csum[FW];
    __shared__ double wmin[FW];
    // the slice table's block-wide part (instances without it reference none of these)
    __shared__ uint32_t tot[NB + 1];       // arrivals of all streams before slice b
    __shared__ uint32_t slbad;             // the replica takes the search loop
    // (cum_at masks a slice index with NB / 2 - 1: a power of two)
    static_assert(NB == 0 || (LPS == 2 && NB >= 4 && (NB & (NB - 1)) == 0 && NB <= 64 && NB * 32 * 4 <= FCAP * 8),
                  "slice table");

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int64_t rl = blockIdx.x;
    const int s = tid / LPS, k = tid % LPS, g0l = lane & ~(LPS - 1);
    const double* rep = a.streams + rl * a.capsum;
    int L = 0;
    uint32_t off = 0;
    if (s < a.n_str) {
        L = a.slen[(int64_t)s * a.slen_stride + rl];
        off = (uint32_t)a.st_off[s];
    }
    int cur = 0;
    double head = RQ_INF;
    if (k == 0 && L > 0) head = rep[off];
#pragma unroll
    for (int q = 0; q < PT; ++q) cnt[tid + q * FB] = 0;
    {
        const double m = wave_min_f64(head);
        const uint32_t sm = wave_sum_u32(k == 0 ? (uint32_t)L : 0u);
        if (lane == 0) {
            wmin[w] = m;
            wsum[0][w] = sm;
        }
    }
    __syncthreads();
    double t_lo = wmin[0];
    uint32_t total = 0;
#pragma unroll
    for (int q = 0; q < FW; ++q) {
        t_lo = wmin[q] < t_lo ? wmin[q] : t_lo;
        total += wsum[0][q];
    }
    double span = (a.end - t_lo) * ((double)FTARGET / (double)(total > 1 ? total : 1));
    int64_t outpos = 0;
    double* out_t = a.out_t + rl * a.mrg_stride;
    uint16_t* out_j = a.out_j + rl * a.mrg_stride;
    int status = 0;
    int par = 1;   // wsum[par]: a retried window's sums are written while the last ones are read
#ifdef RQ_PHASE_CLOCK
    // diagnostic builds: thread 0's view of where a block's time goes (a.clk, scripts/dev/flat_clock.py)
    unsigned long long ck[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tc0 = __builtin_amdgcn_s_memtime(), tc1 = 0;
#define RQ_FLAT_TICK(q)                                                  \
    do {                                                                 \
        tc1 = __builtin_amdgcn_s_memtime();                              \
        ck[q] += tc1 - tc0;                                              \
        tc0 = tc1;                                                       \
    } while (0)
#else
#define RQ_FLAT_TICK(q) do { } while (0)
#endif

    // One window: the nr arrivals in [w_lo, w_hi) -- stream s2's run starts at sbase[s2] and
    // pre[s2] items come before it (both in LDS, a barrier behind them) -- through the item
    // pass and (a)-(d).  `mid` runs between the scatter and its barrier.
    auto window = [&](const double w_lo, const double w_hi, const uint32_t nr, auto&& mid) {
        // ---- the window's items into registers; (a) histogram ----
        const double scale = (double)FM / (w_hi - w_lo);
        double tv[PT];
        uint32_t kv[PT];
#pragma unroll
        for (int q = 0; q < PT; ++q) {
            // unconditional (a slot past the window repeats its last item and drops it below):
            // the PT searches interleave, and no load waits behind a branch
            const uint32_t i0 = (uint32_t)(tid + q * FB), i = i0 < nr ? i0 : nr - 1u;
            uint32_t s2 = 0;   // the last stream with pre <= i (empty streams repeat a value)
#pragma unroll
            for (uint32_t step = 32; step > 0; step >>= 1) s2 += pre[s2 + step] <= i ? step : 0u;
            const uint32_t pos = i - pre[s2];
            tv[q] = rep[sbase[s2] + pos];
            kv[q] = (s2 << KB) | pos;
        }
#ifdef RQ_PHASE_CLOCK
        __builtin_amdgcn_s_waitcnt(0);   // the item loads' round trip on its own tick
        RQ_FLAT_TICK(2);
#endif
#pragma unroll
        for (int q = 0; q < PT; ++q) {
            if ((uint32_t)(tid + q * FB) < nr) {
                const uint32_t sb = (uint32_t)flat_sub<FM>(tv[q], w_lo, scale);
                atomicAdd(&cnt[sb], 1u);
                kv[q] |= sb << SB_SH;
            }
        }
        __syncthreads();
        // ---- (b) bucket bases: exclusive scan of cnt in place (PT buckets per thread) ----
        {
            uint32_t v[PT], tsum = 0;
#pragma unroll
            for (int q = 0; q < PT; q += 4) {
                const uint4 x = *reinterpret_cast<const uint4*>(&cnt[PT * tid + q]);
                v[q] = x.x, v[q + 1] = x.y, v[q + 2] = x.z, v[q + 3] = x.w;
                tsum += x.x + x.y + x.z + x.w;
            }
            const uint32_t ci = wave_scan_add(tsum);
            if (lane == 63) csum[w] = ci;
            __syncthreads();
            uint32_t b = ci - tsum;
#pragma unroll
            for (int q = 0; q < FW; ++q) b += q < w ? csum[q] : 0u;
#pragma unroll
            for (int q = 0; q < PT; q += 4) {
                uint4 x;
                x.x = b, x.y = b + v[q], x.z = x.y + v[q + 1], x.w = x.z + v[q + 2];
                b = x.w + v[q + 3];
                *reinterpret_cast<uint4*>(&cnt[PT * tid + q]) = x;
            }
        }
        __syncthreads();
        // ---- (c) into bucket order: a bucket's base is its cursor, and ends as its end ----
#pragma unroll
        for (int q = 0; q < PT; ++q) {
            if ((uint32_t)(tid + q * FB) < nr) {
                const uint32_t pos = atomicAdd(&cnt[kv[q] >> SB_SH], 1u);
                st[pos] = tv[q];
                sk[pos] = kv[q] & ((1u << SB_SH) - 1u);
            }
        }
        mid();
        __syncthreads();
        RQ_FLAT_TICK(3);
        // ---- (d) rank inside the bucket, written out in play order ----
        for (int i = tid; i < (int)nr; i += FB) {
            const double x = st[i];
            const uint32_t kx = sk[i];
            const int sb = flat_sub<FM>(x, w_lo, scale);
            const int g0 = sb > 0 ? (int)cnt[sb - 1] : 0, g1 = (int)cnt[sb];
            int r = 0;
            for (int q = g0; q < g1; ++q) {
                const double y = st[q];
                r += (y < x || (y == x && sk[q] < kx)) ? 1 : 0;
            }
            // streaming stores, as the bucket rounds': the output must not evict the input
            __builtin_nontemporal_store(x, &out_t[outpos + g0 + r]);
            __builtin_nontemporal_store((uint16_t)(kx >> KB), &out_j[outpos + g0 + r]);
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < PT; ++q) cnt[tid + q * FB] = 0;   // the next histogram is two barriers away
        RQ_FLAT_TICK(6);
#ifdef RQ_PHASE_CLOCK
        ck[4] += 1;
#endif
    };

    bool by_table = false;
    if constexpr (NB > 0) {
        // a replica with nothing before the horizon's end has no window either way; one whose
        // arrivals do not fit the merged capacity stops where the search loop's windows stop
        // (out_len and the emitted prefix of an RQ_ST_STREAM_OVERFLOW replica are that loop's)
        if (total > 0 && t_lo <= a.end && (int64_t)total <= a.mrg_stride) {
            constexpr int HW = NB / 2;   // count words per stream: two 16-bit slice counts each
            constexpr int CW = NB / 4;   // cum words per lane: the stream's lane k holds boundaries [k HW, k HW + HW)
            // hist[g / 2][s]: the counts of slices g (even: low half) and g + 1 of stream s; it
            // lies in st, which no window has written yet
            uint32_t* hist = reinterpret_cast<uint32_t*>(st);
            const double t_min = t_lo, wid = a.end - t_min;
            for (int q = tid; q < HW * 64; q += FB) hist[q] = 0;
            if (tid == 0) slbad = 0;
            __syncthreads();
            // ---- the pre-pass: lane k of a stream reads its 32-byte chunks k, k + 2, ... ----
            const double inv = wid > 0.0 ? (double)NB / wid : 0.0;
            // (past 65,535 arrivals a stream's 16-bit slice count could carry into its neighbour's
            // half of the word, and the totals would no longer show the slice over FCAP)
            bool bad = L > 65535;
            const int nch = (L + 3) >> 2, lastc = L > 0 ? (L - 1) & ~3 : 0;   // loads stay inside the last chunk
            const double4* src4 = reinterpret_cast<const double4*>(rep + off);   // capacities are whole lines
            double carry = -RQ_INF;   // lane 0: the entry before its chunk (the neighbour's last)
            constexpr int BT = RQ_FLAT_BT;   // chunks in flight per lane
            for (int c0 = 0; c0 < nch; c0 += 2 * BT) {   // the two lanes of a stream run together
                double4 v[BT];
#pragma unroll
                for (int b = 0; b < BT; ++b) {
                    const int i4 = 4 * (c0 + 2 * b + k);
                    v[b] = src4[(i4 < lastc ? i4 : lastc) >> 2];
                }
#pragma unroll
                for (int b = 0; b < BT; ++b) {
                    const int i4 = 4 * (c0 + 2 * b + k);
                    const double nbw = flat_swap1_f64(v[b].w);
                    const double pv = k ? nbw : carry;
                    carry = nbw;
                    const double e[5] = {pv, v[b].x, v[b].y, v[b].z, v[b].w};
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        if (i4 + q < L) {
                            const double t = e[q + 1];
                            bad |= !(t >= t_min && t <= a.end) || t < e[q];
                            const double x0 = (t - t_min) * inv, x = x0 > 0.0 ? x0 : 0.0;
                            int g = x < (double)(NB - 1) ? (int)x : NB - 1;
                            atomicAdd(&hist[(g >> 1) * 64 + s], 1u << ((g & 1) * 16));
                        }
                    }
                }
            }
            if (bad) slbad = 1;
            __syncthreads();
            // ---- cum: lane k's half of the stream's counts, summed from the stream's start ----
            uint32_t cw[CW];
            {
                uint32_t run = 0;
#pragma unroll
                for (int r = 0; r < CW; ++r) {
                    const uint32_t h = hist[(k * CW + r) * 64 + s];
                    cw[r] = run | ((run + (h & 0xFFFFu)) << 16);
                    run += (h & 0xFFFFu) + (h >> 16);
                }
                const uint32_t nbrun = flat_swap1(run);   // (both lanes active: a DPP read of an idle lane gives 0)
                const uint32_t first = k ? nbrun : 0u;    // lane 1: what lane 0's half holds
#pragma unroll
                for (int r = 0; r < CW; ++r) cw[r] += first | (first << 16);
            }
            // ---- tot: thread b sums slice b over the streams (rotated: no two words of a step share a bank) ----
            if (w == 0) {
                uint32_t sl = 0;
                if (tid < NB)
#pragma unroll 16
                    for (int q = 0; q < 64; ++q)
                        sl += (hist[(tid >> 1) * 64 + ((q + (tid >> 1)) & 63)] >> ((tid & 1) * 16)) & 0xFFFFu;
                if (sl > (uint32_t)FCAP) slbad = 1;
                const uint32_t ti = wave_scan_add(sl);
                if (tid < NB) tot[tid + 1] = ti;
                if (tid == 0) tot[0] = 0;
            }
            __syncthreads();
            RQ_FLAT_TICK(7);
            // cum[s][b] in both lanes of stream s (b is block-uniform: the selects are scalar-controlled)
            auto cum_at = [&](const int b) -> uint32_t {
                const int idx = b & (HW - 1);
                // a tree of selects on the index's bits (indexing cw would put it in scratch memory)
                uint32_t y4[CW];
#pragma unroll
                for (int r = 0; r < CW; ++r) y4[r] = cw[r];
#pragma unroll
                for (int h = 1; h < CW; h <<= 1)
#pragma unroll
                    for (int r = 0; r < CW; r += 2 * h) y4[r] = ((idx >> 1) & h) ? y4[r + h] : y4[r];
                uint32_t x = y4[0];
                x = (idx & 1) ? x >> 16 : x & 0xFFFFu;
                const uint32_t y = flat_swap1(x);
                return b >= NB ? (uint32_t)L : ((b >= HW) == (k != 0) ? x : y);
            };
            auto tot_at = [&](const int b) -> uint32_t { return (uint32_t)__builtin_amdgcn_readfirstlane((int)tot[b]); };
            if (!__builtin_amdgcn_readfirstlane((int)slbad)) {
                by_table = true;
                int b0 = 0;
                while (b0 < NB) {
                    // the longest run of slices from b0 that a window holds (every slice alone does)
                    const uint32_t tb0 = tot_at(b0);
                    int b1 = b0 + 1;
                    while (b1 < NB && tot_at(b1 + 1) - tb0 <= (uint32_t)FCAP) ++b1;
                    const uint32_t nr = tot_at(b1) - tb0;
                    if (outpos + (int64_t)nr > a.mrg_stride) {   // past the merged capacity (uniform)
                        status |= RQ_ST_STREAM_OVERFLOW;
                        break;
                    }
                    if (nr == 0) {   // empty slices to the end
                        b0 = b1;
                        continue;
                    }
                    const uint32_t c0 = cum_at(b0), ns = cum_at(b1) - c0;
                    const uint32_t incl = wave_scan_add(k == 0 ? ns : 0u);
                    if (lane == 63) wsum[par][w] = incl;
                    __syncthreads();
                    uint32_t wo = 0;
#pragma unroll
                    for (int q = 0; q < FW; ++q) wo += q < w ? wsum[par][q] : 0u;
                    par ^= 1;
                    if (k == 0) {
                        pre[s] = wo + incl - ns;
                        sbase[s] = off + c0;
                    }
                    RQ_FLAT_TICK(0);
                    __syncthreads();
                    RQ_FLAT_TICK(1);
                    // the sub-buckets' range only shapes the window's internal sort
                    window(t_min + wid * ((double)b0 / (double)NB), b1 < NB ? t_min + wid * ((double)b1 / (double)NB) : a.end,
                           nr, []() {});
                    outpos += nr;
                    b0 = b1;
                }
            }
#ifdef RQ_PHASE_CLOCK
            else
                ck[5] += 1ull << 32;   // a replica on the search loop
#endif
        }
    }

    if (!by_table) {
    while (t_lo <= a.end) {
        double tau = t_lo + span;
        if (!(tau > t_lo)) tau = next_up(t_lo);
        // ---- the stream's run [cur, lo): its arrivals before tau ----
        // invariant: entries below lo are before tau, entries from hi on are not
        int lo = cur, hi = L;
        for (;;) {
            const int n = hi - lo;
            const bool act = n > 0;
            if (!__ballot(act)) break;
            // probes lo + n (k + 1) / (LPS + 1) < hi, non-decreasing in k
            const uint32_t un = (uint32_t)(act ? n : 0);
            bool below = false;
            if (act) below = rep[off + (uint32_t)lo + un * (uint32_t)(k + 1) / (uint32_t)(LPS + 1)] < tau;
            const uint64_t bal = __ballot(below);
            const uint32_t c = (uint32_t)__popc((uint32_t)(bal >> g0l) & ((1u << LPS) - 1u));   // a prefix of the probes
            if (act) {
                if (c < (uint32_t)LPS) hi = lo + (int)(un * (c + 1u) / (uint32_t)(LPS + 1));
                if (c > 0) lo = lo + (int)(un * c / (uint32_t)(LPS + 1)) + 1;
            }
        }
        const int ns = lo - cur;
        const uint32_t incl = wave_scan_add(k == 0 ? (uint32_t)ns : 0u);
        if (lane == 63) wsum[par][w] = incl;
        __syncthreads();
        uint32_t wo = 0, nr_all = 0;
#pragma unroll
        for (int q = 0; q < FW; ++q) {
            const uint32_t v = wsum[par][q];
            wo += q < w ? v : 0u;
            nr_all += v;
        }
        par ^= 1;
        uint32_t nr = nr_all;
        if (nr_all > (uint32_t)FCAP) {
            if (tau != next_up(t_lo)) {   // too many for one window: halve the cut (nothing to undo)
                span = (tau - t_lo) * 0.5;
#ifdef RQ_PHASE_CLOCK
                ck[5] += 1;
#endif
                RQ_FLAT_TICK(0);
                continue;
            }
            // more than FCAP arrivals at t_lo itself: the first FCAP in (stream, position)
            // order (any subset of equal times is a time prefix), and flag the replica
            nr = FCAP;
            status |= a.strict_ties ? RQ_ST_UNORDERED : RQ_ST_TIE;
        }
        if (outpos + (int64_t)nr > a.mrg_stride) {   // past the merged capacity (uniform)
            status |= RQ_ST_STREAM_OVERFLOW;
            break;
        }
        if (nr == 0) break;   // (the head at t_lo is before tau: only unordered input gets here)
        RQ_FLAT_TICK(0);
        {
            // the group's lanes hold the same incl - ns: the items before their stream
            const uint32_t e0 = wo + incl - (uint32_t)ns;
            const int room = e0 < nr ? (int)(nr - e0) : 0;
            if (k == 0) {
                pre[s] = e0;
                sbase[s] = off + (uint32_t)cur;
            }
            cur += ns < room ? ns : room;
            head = RQ_INF;
            if (k == 0 && cur < L) head = rep[off + (uint32_t)cur];   // used after the scatter
        }
        __syncthreads();
        RQ_FLAT_TICK(1);
        window(t_lo, tau, nr, [&]() {
            const double m = wave_min_f64(head);
            if (lane == 0) wmin[w] = m;
        });
        double t_next = wmin[0];
#pragma unroll
        for (int q = 1; q < FW; ++q) t_next = wmin[q] < t_next ? wmin[q] : t_next;
        outpos += nr;
        // next cut: aim at FTARGET arrivals, grow at most 4x per window
        const double wdt = tau - t_lo;
        const double f = (double)FTARGET / (double)(nr > 64 ? nr : 64);
        span = wdt * (f < 4.0 ? f : 4.0);
        t_lo = t_next;   // the heads after the window (an equal-time window: t_lo again)
    }
    }
#ifdef RQ_PHASE_CLOCK
    // phases: 0 run search (table: cum selects + scan), 1 pre / sbase and their barriers, 2 item
    // loads, 3 histogram + scan + scatter, 6 rank + write-out, 7 the table's pre-pass; 4 windows,
    // 5 retried windows + (replicas on the search loop << 32)
    if (a.clk && tid == 0)
        for (int q = 0; q < 8; ++q) atomicAdd(&a.clk[q], ck[q]);
#endif
#undef RQ_FLAT_TICK
    if (tid == 0) {
        a.out_len[rl] = (int)outpos;
        if (status) atomicOr(&a.status[a.chunk0 + rl], status);
    }
}

// A handful of streams (C4 / C2: the README graph's three, ~2100 arrivals per replica):
// the bucket rounds ran a 64-lane block with 3 lanes walking, so here the merge is a
// RANKING instead.  A block stages its replica's streams in LDS (coalesced), then every
// arrival finds its place in the play order at once: its index in its own stream plus,
// per other stream j', the arrivals of j' that play before it -- those at an earlier
// time, or at the same time when j' < j (equal times in stream order, as the bucket
// rounds emit them) -- by binary search in LDS, and is written there.  No equal-time
// cap; the same (t, stream) sequence.
template <int NS>
__global__ __launch_bounds__(256) void rq_merge_rank(MergeArgs a)
{
    extern __shared__ double mr_sh[];
    const int64_t rl = blockIdx.x;
    const int tid = threadIdx.x;
    const double* base = a.streams + rl * a.capsum;
    int len[NS], off[NS];
    int64_t total = 0;
#pragma unroll
    for (int j = 0; j < NS; ++j) {
        len[j] = j < a.n_str ? a.slen[(int64_t)j * a.slen_stride + rl] : 0;
        off[j] = j < a.n_str ? (int)a.st_off[j] : 0;
        total += len[j];
    }
#pragma unroll
    for (int j = 0; j < NS; ++j)
        for (int i = tid; i < len[j]; i += blockDim.x) mr_sh[off[j] + i] = base[off[j] + i];
    __syncthreads();
    double* ot = a.out_t + rl * a.mrg_stride;
    uint16_t* oj = a.out_j + rl * a.mrg_stride;
#pragma unroll
    for (int j = 0; j < NS; ++j) {
        for (int i = tid; i < len[j]; i += blockDim.x) {
            const double t = mr_sh[off[j] + i];
            int64_t r = i;
#pragma unroll
            for (int q = 0; q < NS; ++q) {
                if (q == j || len[q] == 0) continue;
                // arrivals of stream q before t: t' < t, or t' <= t for q < j
                const double* v = mr_sh + off[q];
                int lo = 0, hi = len[q];
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    const double x = v[mid];
                    if (x < t || (q < j && x == t)) lo = mid + 1;
                    else hi = mid;
                }
                r += lo;
            }
            // plain stores: the inputs are in LDS (nothing to protect in L2), and the
            // scattered 8-B / 2-B entries of a line merge in L2 before the write-back
            // (nontemporal stores wrote 2.0 x the 10 B per entry; C4 27.7 -> 25.9 ms)
            if (r < a.mrg_stride) {
                ot[r] = t;
                oj[r] = (uint16_t)j;
            }
        }
    }
    if (tid == 0) {
        a.out_len[rl] = (int)(total < a.mrg_stride ? total : a.mrg_stride);
        if (total > a.mrg_stride) atomicOr(&a.status[a.chunk0 + rl], RQ_ST_STREAM_OVERFLOW);
    }
}

hipError_t rq_launch_merge(const MergeArgs& a, hipStream_t s)
{
    if (a.n_chunk <= 0) return hipSuccess;
    if (a.n_str > RQ_MG_B) return hipErrorInvalidValue;
    const char* e = getenv("RQ_MERGE_SMALL");   // A/B and the bucket merge's own tests only
    const bool small_on = !e || atoi(e) != 0;
    // <= 8 streams whose buffers fit a block's LDS: the ranking merge
    const size_t lds = (size_t)a.capsum * sizeof(double);
    if (small_on && a.n_str <= 8 && lds <= 64 * 1024) {
        if (a.n_str <= 4)
            hipLaunchKernelGGL((rq_merge_rank<4>), dim3((unsigned)a.n_chunk), dim3(256), lds, s, a);
        else
            hipLaunchKernelGGL((rq_merge_rank<8>), dim3((unsigned)a.n_chunk), dim3(256), lds, s, a);
        return hipGetLastError();
    }
    // <= 64 streams: flat windows, unless the ranking merge was switched off (RQ_MERGE_SMALL=0
    // means the bucket rounds, whose own tests set it) or RQ_MERGE_FLAT=0 (A/B and tests)
    const char* ef = getenv("RQ_MERGE_FLAT");
    const int flat = ef ? atoi(ef) : 1;
    if (small_on && flat != 0 && a.n_str <= 64 && a.capsum < ((int64_t)1 << 31)) {
        // RQ_FLAT_SLICES=0: the search loop for every replica (A/B and tests)
        const char* es = getenv("RQ_FLAT_SLICES");
        const int slices = es ? atoi(es) : 1;
#define RQ_FLAT_LAUNCH(FB, FCAP, FT8, NB) \
    hipLaunchKernelGGL((rq_merge_flat<FB, FCAP, FT8, NB>), dim3((unsigned)a.n_chunk), dim3(FB), 0, s, a)
#ifdef RQ_FLAT_SHAPES
        // tuning builds (EXTRA=-DRQ_FLAT_SHAPES): RQ_MERGE_FLAT = waves * 100000 + window
        // capacity * 10 + eighths of it a window aims at (DESIGN 22 has the measurements)
        switch (flat) {
        case 102566: RQ_FLAT_LAUNCH(64, 256, 6, 0); return hipGetLastError();
        case 105126: RQ_FLAT_LAUNCH(64, 512, 6, 0); return hipGetLastError();
        case 205126: RQ_FLAT_LAUNCH(128, 512, 6, 0); return hipGetLastError();
        case 210245: RQ_FLAT_LAUNCH(128, 1024, 5, 0); return hipGetLastError();
        case 210246: RQ_FLAT_LAUNCH(128, 1024, 6, 0); return hipGetLastError();
        case 215366: RQ_FLAT_LAUNCH(128, 1536, 6, 0); return hipGetLastError();
        case 220486: RQ_FLAT_LAUNCH(128, 2048, 6, 0); return hipGetLastError();
        case 410246: RQ_FLAT_LAUNCH(256, 1024, 6, 0); return hipGetLastError();
        case 410247: RQ_FLAT_LAUNCH(256, 1024, 7, 0); return hipGetLastError();
        case 420486: RQ_FLAT_LAUNCH(256, 2048, 6, 0); return hipGetLastError();
        case 430726: RQ_FLAT_LAUNCH(256, 3072, 6, 0); return hipGetLastError();
        case 820486: RQ_FLAT_LAUNCH(512, 2048, 6, 0); return hipGetLastError();
        default: break;
        }
        // ... and RQ_FLAT_SLICES = the slice count of the launched shape's table
        switch (slices) {
        case 16: RQ_FLAT_LAUNCH(128, 1024, 7, 16); return hipGetLastError();
        case 32: RQ_FLAT_LAUNCH(128, 1024, 7, 32); return hipGetLastError();
        case 64: RQ_FLAT_LAUNCH(128, 1024, 7, 64); return hipGetLastError();
        default: break;
        }
#endif
        if (slices != 0)
            RQ_FLAT_LAUNCH(128, 1024, 7, RQ_FLAT_NB);
        else
            RQ_FLAT_LAUNCH(128, 1024, 7, 0);
#undef RQ_FLAT_LAUNCH
        return hipGetLastError();
    }
    if (a.n_str <= 64)
        hipLaunchKernelGGL((rq_merge_streams<64, false>), dim3((unsigned)a.n_chunk), dim3(64), 0, s, a);
    else
        hipLaunchKernelGGL((rq_merge_streams<RQ_MG_B, false>), dim3((unsigned)a.n_chunk), dim3(RQ_MG_B), 0, s, a);
    return hipGetLastError();
}

hipError_t rq_launch_merge_groups(const MergeArgs& a, hipStream_t s)
{
    if (a.n_chunk <= 0) return hipSuccess;
    if (a.grp_sz != 64 && a.grp_sz != RQ_MG_B) return hipErrorInvalidValue;
    const int ng = (a.n_str + a.grp_sz - 1) / a.grp_sz;
    if (ng < 2 || ng > RQ_MG_B || a.n_str > RQ_MAX_STREAMS_MRG) return hipErrorInvalidValue;
    if (a.grp_sz == 64)
        hipLaunchKernelGGL((rq_merge_streams<64, false>), dim3((unsigned)a.n_chunk, (unsigned)ng), dim3(64), 0, s, a);
    else
        hipLaunchKernelGGL((rq_merge_streams<RQ_MG_B, false>), dim3((unsigned)a.n_chunk, (unsigned)ng), dim3(RQ_MG_B), 0,
                           s, a);
    return hipGetLastError();
}

hipError_t rq_launch_merge_sub(const MergeArgs& a, hipStream_t s)
{
    if (a.n_chunk <= 0) return hipSuccess;
    if (a.n_grp < 1 || a.n_grp > RQ_MG_B || !a.sub_t || !a.sub_j || !a.sub_len) return hipErrorInvalidValue;
    // <= 64 groups are <= 32768 streams: 16-bit ids; past 65535 streams the WIDE instance
    if (a.n_grp <= 64) {
        hipLaunchKernelGGL((rq_merge_streams<64, true>), dim3((unsigned)a.n_chunk), dim3(64), 0, s, a);
    } else if (a.out_jh) {
        hipLaunchKernelGGL((rq_merge_streams<RQ_MG_B, true, true>), dim3((unsigned)a.n_chunk), dim3(RQ_MG_B), 0, s, a);
    } else {
        hipLaunchKernelGGL((rq_merge_streams<RQ_MG_B, true>), dim3((unsigned)a.n_chunk), dim3(RQ_MG_B), 0, s, a);
    }
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Longest-first replica order for the sweeps' work queues (LPT): the sweep of a
// replica costs about its merged length, and the waves take replicas in queue order,
// so the longest go first and the launch ends on short ones.  One wave (it must find a
// slot while another stream's sweep holds the chip): a counting sort of the lengths
// into OB buckets of (max - len) (descending length; replicas of one bucket in any
// order -- outputs are indexed by replica, so the order changes no result bit, only
// which wave plays which replica when).
// ---------------------------------------------------------------------------
namespace {
constexpr int OB = 1024;   // buckets (16 per lane)
}

__global__ __launch_bounds__(64) void rq_order_replicas(const int* __restrict__ len, int n, int* __restrict__ order)
{
    __shared__ uint32_t hist[OB];
    const int lane = threadIdx.x;
    int mn = 0x7fffffff, mx = 0;
    for (int i = lane; i < n; i += 64) {
        const int v = len[i];
        mn = v < mn ? v : mn;
        mx = v > mx ? v : mx;
    }
    for (int k = lane; k < OB; k += 64) hist[k] = 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int a = __shfl_xor(mn, o), b = __shfl_xor(mx, o);
        mn = a < mn ? a : mn;
        mx = b > mx ? b : mx;
    }
    const int64_t span = (int64_t)mx - mn + 1;
    auto bucket = [&](int v) -> int { return (int)(((int64_t)(mx - v) * OB) / span); };
    wave_lds_sync();
    for (int i = lane; i < n; i += 64) atomicAdd(&hist[bucket(len[i])], 1u);
    wave_lds_sync();
    // exclusive scan: lane l owns buckets [16 l, 16 l + 16)
    uint32_t h[OB / 64], sum = 0;
#pragma unroll
    for (int k = 0; k < OB / 64; ++k) {
        h[k] = hist[lane * (OB / 64) + k];
        sum += h[k];
    }
    uint32_t base = wave_scan_add(sum) - sum;
#pragma unroll
    for (int k = 0; k < OB / 64; ++k) {
        hist[lane * (OB / 64) + k] = base;
        base += h[k];
    }
    wave_lds_sync();
    for (int i = lane; i < n; i += 64) order[atomicAdd(&hist[bucket(len[i])], 1u)] = i;
}

hipError_t rq_launch_order(const int* len, int64_t n, int* order, hipStream_t s)
{
    if (n <= 0) return hipSuccess;
    if (n > 65536) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rq_order_replicas, dim3(1), dim3(64), 0, s, len, (int)n, order);
    return hipGetLastError();
}

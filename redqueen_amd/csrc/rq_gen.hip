// rq_gen.hip -- the arrival streams of a chunk, written to HBM for the merge and the sweeps.
//
// One lane per (replica, stream), 256 replicas of ONE stream per block, so a block never
// diverges on the source kind.  The graph's streams are in three classes (GraphTopo.gen_cls)
// and a block of rq_gen_classes branches, block-uniformly, into its class's body:
//   H  Hawkes :466-490 -- SrcGen's step machine with the kind a template constant (no kind
//      tests, straight-line logarithms)
//   P  Poisson :424-433, Poisson2 :396-405 (the controlled stream too when it is a Poisson
//      broadcaster) -- 16 arrivals per trip: a Poisson stream has no serial chain but the
//      running sum, and arrival k of a chunk goes to slot k in every lane
//   G  PiecewiseConst :642-663, RealData :722-750, the empty controlled slot -- SrcGen::step
//      as it is
// rq_gen_streams (RQ_GEN_SPLIT=0) is the G body for every stream.  All of them write the bits
// SrcGen::step gives (rq_gen.h; the fused sweep calls it itself).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rq_device.h"
#include "rq_internal.h"
#include "rq_gen.h"
#include <algorithm>

#pragma clang fp contract(off)

using namespace rq;

namespace {

// a launch's rows: row r < ln is stream cls[l0 + r] of the graph's class list, row ln
// (rows == ln + 1) the controlled stream, whose class depends on the call.  No list: row r
// is stream r.  More than 32768 rows fold into z.
struct GenRows {
    int l0, ln, rows;
};
__device__ __forceinline__ int gen_row() { return (int)(blockIdx.z * gridDim.y + blockIdx.y); }
__device__ __forceinline__ int gen_stream(const GenArgs& a, const GenRows& g, int r)
{
    return a.cls ? (r < g.ln ? a.cls[g.l0 + r] : a.ctrl_idx) : r;
}

// rq_exp's table in LDS: a Hawkes candidate's exp looks up two per-lane words in its
// dependent chain (from __constant__ memory these were vector loads at L1/L2 latency)
__device__ __forceinline__ void gen_load_etab(uint64_t* etab)
{
    for (int e = threadIdx.x; e < RQ_EXP_TAB_N; e += blockDim.x) etab[e] = rq_exp_tab_c[e];
    __syncthreads();
}

// stream j of chunk replica rl, one candidate per trip
template <int KIND>
__device__ __forceinline__ void gen_steps(const GenArgs& a, int j, int64_t rl, const uint64_t* etab)
{
    const int64_t o = a.chunk0 + rl;      // local output index
    const int64_t i = rq_replica_of(a, o);   // global id (seeds)
    SrcGenT<KIND> gen;
    gen.init(a, j, i, etab);

    double* out = a.streams + rl * a.capsum + a.st_off[j];   // 128-byte aligned (host pads)
    const int cap = a.cap[j];                                   // multiple of 16
    int n = 0;
    bool ovf = false;
    // arrivals are staged RQ_GEN_W at a time in registers (compile-time shift, no
    // scratch) and written as one lane-contiguous chunk: 16 = a whole 128-byte line per
    // lane, so no line is written in halves at different times (C3: written bytes 1.22 ->
    // 1.04 x the 8 B per arrival; 8: gen 5 % faster at 90 instead of 106 VGPRs)
#ifndef RQ_GEN_W
#define RQ_GEN_W 16
#endif
    constexpr int GW = RQ_GEN_W;
    static_assert(GW == 8 || GW == 16, "staging width");
    double sb[GW];
#pragma unroll
    for (int k = 0; k < GW; ++k) sb[k] = 0.0;
    while (!gen.done && !ovf) {
        double tv;
        if (gen.step(&tv, a.end)) {
            if (n < cap) {
#pragma unroll
                for (int k = 0; k + 1 < GW; ++k) sb[k] = sb[k + 1];
                sb[GW - 1] = tv;
                ++n;
                if ((n & (GW - 1)) == 0) {
                    double4* d = reinterpret_cast<double4*>(out + n - GW);
#pragma unroll
                    for (int k = 0; k < GW / 4; ++k) d[k] = make_double4(sb[4 * k], sb[4 * k + 1], sb[4 * k + 2], sb[4 * k + 3]);
                }
            } else {
                ovf = true;
            }
        }
    }
    {   // the last partial chunk: values sit in sb[GW-r .. GW-1]; written as one whole
        // chunk (slots past n hold stale values nobody reads: readers stop at slen)
        const int r = n & (GW - 1);
        if (r > 0) {
            // shift the staged values left by GW - r (log-steps of static shifts: no scratch).
            // RQ_GEN_TAIL_STEPS: each step selects between two VALUES per slot, GW x log2 GW
            // two-way selects in all.  0 (A/B): the select between two array elements, an
            // lvalue the compiler turns into one element at a selected index -- a GW-way
            // compare-and-select chain per output word and step
#ifndef RQ_GEN_TAIL_STEPS
#define RQ_GEN_TAIL_STEPS 1
#endif
            const int sh = GW - r;
#pragma unroll
            for (int st = 1; st < GW; st <<= 1) {
                const bool on = (sh & st) != 0;
#pragma unroll
                for (int k = 0; k < GW; ++k) {
#if RQ_GEN_TAIL_STEPS
                    const double up = sb[k + st < GW ? k + st : GW - 1], keep = sb[k];
                    sb[k] = on ? up : keep;
#else
                    sb[k] = on ? sb[k + st < GW ? k + st : GW - 1] : sb[k];
#endif
                }
            }
            // whole 64-byte halves, only those holding arrivals
            double4* d = reinterpret_cast<double4*>(out + (n - r));
#pragma unroll
            for (int k = 0; k < GW / 4; ++k)
                if (k < 2 || r > 8) d[k] = make_double4(sb[4 * k], sb[4 * k + 1], sb[4 * k + 2], sb[4 * k + 3]);
        }
    }
    a.slen[(int64_t)j * a.slen_stride + rl] = n;   // consecutive lanes, consecutive ints
    if (ovf) atomicOr(&a.status[o], RQ_ST_STREAM_OVERFLOW);
}

// Poisson / Poisson2 stream j of chunk replica rl, 16 arrivals per trip.  Draw d of the
// stream is half d & 1 of Philox call d >> 1 and every candidate up to the end is an arrival,
// so chunk c is calls 8 c .. 8 c + 7: sixteen independent exponentials, and only the running
// sum t_k = t_(k-1) + e_k * inv is serial (formed in step()'s order, so the same bits).
// Arrival k of a chunk sits in sb[k] in every lane: no staging shifts, and the last, partial
// chunk is in place.  The sixteen logarithms are straight-line code (gen_exponential).
__device__ __forceinline__ void gen_poisson(const GenArgs& a, int j, int64_t rl)
{
    const int64_t o = a.chunk0 + rl;
    const int64_t i = rq_replica_of(a, o);
    const bool is_ctrl = j == a.ctrl_idx;
    const uint32_t k0 = gen_seed(a, j, i, is_ctrl);
    const uint32_t k1 = kind_salt(is_ctrl ? a.ctrl_stream_kind : a.kind[j], is_ctrl);
    const double rate = is_ctrl ? a.ctrl_rate[i] : a.p0[j];
    const double end = a.end;
    double* out = a.streams + rl * a.capsum + a.st_off[j];   // 128-byte aligned (host pads)
    const int cap = a.cap[j];                                   // multiple of 16
    bool done = !(rate > 0.0), ovf = false;
    const double inv = done ? 0.0 : 1.0 / rate;
    double t = a.start;
    int n = 0;   // arrivals stored in whole chunks = draws taken
    while (!done) {
        if (n >= cap) {
            // the stream is full: step() draws one more candidate (draw n, the first half of
            // a call) and flags the overflow if it is an arrival
            uint32_t c[4] = {(uint32_t)n >> 1, 0u, 0u, 0u};
            philox4x32_10(c, k0, k1);
            const double tc = t + gen_exponential(c[0], c[1]) * inv;
            ovf = tc <= end;
            break;
        }
        double sb[16];
        int m = 0;   // leading arrivals of the chunk: !(tc <= end) ends the stream (a NaN too)
        bool ok = true;
        double tc = t;
#pragma unroll
        for (int q = 0; q < 16; q += 2) {
            uint32_t c[4] = {((uint32_t)n + q) >> 1, 0u, 0u, 0u};
            philox4x32_10(c, k0, k1);
            const double e[2] = {gen_exponential(c[0], c[1]), gen_exponential(c[2], c[3])};
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                tc = tc + e[h] * inv;
                ok = ok && tc <= end;
                m += ok ? 1 : 0;
                sb[q + h] = tc;
            }
        }
        // whole 64-byte halves, only those holding arrivals (slots past m hold times past
        // the end that nobody reads: readers stop at slen)
        double4* d = reinterpret_cast<double4*>(out + n);
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < 2 ? m > 0 : m > 8) d[k] = make_double4(sb[4 * k], sb[4 * k + 1], sb[4 * k + 2], sb[4 * k + 3]);
        n += m;
        t = sb[15];
        done = m < 16;
    }
    a.slen[(int64_t)j * a.slen_stride + rl] = n;   // consecutive lanes, consecutive ints
    if (ovf) atomicOr(&a.status[o], RQ_ST_STREAM_OVERFLOW);
}

}  // namespace

__global__ __launch_bounds__(256) void rq_gen_streams(GenArgs a, GenRows g)
{
    __shared__ uint64_t etab[RQ_EXP_TAB_N];
    gen_load_etab(etab);
    const int64_t rl = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int r = gen_row();
    if (rl >= a.n_chunk || r >= g.rows) return;
    gen_steps<-1>(a, gen_stream(a, g, r), rl, etab);
}

// rows [0, h.rows) are class H, the next p.rows class P, the rest class G.  One launch at the
// registers of the largest body: a launch per class (each at its own registers, 5 and 6
// waves per SIMD for H and P) was slower, since a class's grid waits for the last blocks
// of the class before it
__global__ __launch_bounds__(256) void rq_gen_classes(GenArgs a, GenRows h, GenRows p, GenRows g)
{
    __shared__ uint64_t etab[RQ_EXP_TAB_N];
    const int64_t rl = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int r = gen_row();
    if (r >= h.rows + p.rows + g.rows) return;
    if (r < h.rows) {
        gen_load_etab(etab);
        if (rl < a.n_chunk) gen_steps<RQ_SRC_HAWKES>(a, gen_stream(a, h, r), rl, etab);
    } else if ((r -= h.rows) < p.rows) {
        if (rl < a.n_chunk) gen_poisson(a, gen_stream(a, p, r), rl);
    } else {
        gen_load_etab(etab);
        if (rl < a.n_chunk) gen_steps<-1>(a, gen_stream(a, g, r - p.rows), rl, etab);
    }
}

namespace {
template <class K, class... R>
void launch_rows(K k, const GenArgs& a, int rows, hipStream_t s, R... r)
{
    const unsigned gy = (unsigned)std::min(rows, 32768);
    dim3 grid((unsigned)((a.n_chunk + 255) / 256), gy, ((unsigned)rows + gy - 1) / gy);
    hipLaunchKernelGGL(k, grid, dim3(256), 0, s, a, r...);
}
}  // namespace

hipError_t rq_launch_gen(const GenArgs& a, hipStream_t s)
{
    if (a.n_chunk <= 0 || a.n_str <= 0) return hipSuccess;
    if (!a.cls) {   // RQ_GEN_SPLIT=0
        launch_rows(rq_gen_streams, a, a.n_str, s, GenRows{0, a.n_str, a.n_str});
        return hipGetLastError();
    }
    // the controlled stream joins the class of this call's controlled kind.  H rows first:
    // its blocks run longest (1.5 candidates of two draws and an exp per arrival)
    const int ck = a.ctrl_stream_kind;
    const int cc = ck == RQ_SRC_HAWKES ? 0 : (ck == RQ_SRC_POISSON || ck == RQ_SRC_POISSON2) ? 1 : 2;
    GenRows c[3];
    for (int k = 0, l0 = 0; k < 3; l0 += a.cls_n[k], ++k) c[k] = GenRows{l0, a.cls_n[k], a.cls_n[k] + (k == cc ? 1 : 0)};
    launch_rows(rq_gen_classes, a, a.n_str, s, c[0], c[1], c[2]);
    return hipGetLastError();
}

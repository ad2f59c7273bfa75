// rq_log_metrics.hip -- whole-horizon metrics straight from a batch's compact event logs,
// exact on equal times (rq_log_metrics): utils.time_in_top_k / average_rank / int_r_2
// (utils.py:84-121) over the pivot table of rank_of_src_in_df (utils.py:38-56), with the
// fractional cells a (t, sink) pair with several rows has in pandas' pivot mean, plus the
// replay's counts.  No dataframe row is written.
//
// One wavefront per block; a block plays replicas blockIdx.x, + gridDim.x, ... one after
// the other, each in three steps:
//   1. the pivot columns.  A pass over the stream indices marks the streams that occur,
//      a pass over those streams' CSR rows marks their sinks: xbits, one bit per graph
//      sink, and xpre, the set bits below each of its words.  Column of sink x =
//      xpre[x / 32] + popc(xbits[x / 32] below bit x % 32): ascending sink id, the order
//      of the pivot's columns.  S = the set bits.
//   2. the pivot rows.  log_walk (rq_log_walk.h) replays the log against one Cell per
//      column: the rank (next_rank), and the tag, row count and rank sum of the column's
//      last t-group -- its pivot cell is sum / count, carried until the column is touched
//      again (AggX's bookkeeping, rq_sweep_core.h, over the replica's columns instead of
//      the graph's sinks).  Ballots turn the per-lane changes into the deltas of nvalid,
//      c_K, the sum of the integral cells and the number of fractional ones.  When t moves
//      on, the group's row (t, rowsum, nvalid, c_K) is staged, 64 rows to a store, in the
//      block's slot of the workspace; rowsum is the integer sum while no cell is
//      fractional, else numpy's pairwise sum over the S columns (wave_npsum<1>).
//   3. the integrals.  The same wave scans its rows with scan_rows (rq_scan_rows.h): the
//      bits of rq_scan.  Its stores are drained and fenced at workgroup scope first, as
//      in the merged fused sweep's epilogue (rq_sweep_fw.hip).
// Every output element is stored once by lane 0 of its replica's wave.
//
// LDS (rq_log_metrics_lds_bytes): [scratch of wave_npsum<1> / scan_rows][Cell x n_sinks,
// during step 1 the stream bits][xbits][xpre].  A Cell is 16 bytes -- rank i32, tag i32,
// and sum << 24 | count in 64 bits (ev_cap <= 2^20: count <= 2^20, sum < 2^40) -- one
// ds_read_b128 and one ds_write_b128 per row.
#include <hip/hip_runtime.h>

#include "rq_device.h"
#include "rq_internal.h"
#include "rq_log_walk.h"
#include "rq_scan_rows.h"

#pragma clang fp contract(off)

using namespace rq;

namespace {

static_assert(RQ_LM_SCRATCH_BYTES >= 8 * (size_t)npsum_lds_doubles<RQ_MAX_K + 2, RQ_LM_NL>(), "scan_rows scratch");
static_assert(RQ_LM_SCRATCH_BYTES >= 8 * (size_t)npsum_lds_doubles<1>(), "wave_npsum<1> scratch");
static_assert(RQ_LM_SCRATCH_BYTES % 16 == 0, "the cells are read 16 bytes at a time");

struct __attribute__((aligned(16))) Cell {
    int rank, tag;   // next_rank's rank (-1: no row yet); the t-group of the last row (-1: none)
    uint64_t cs;     // that group's rank sum << 24 | its rows
};
static_assert(sizeof(Cell) == RQ_LM_CELL_BYTES, "rq_log_metrics_lds_bytes");

// rows per lane and trip of the scan (TU of wave_npsum_rows), as the fused sweep's fws_tu
constexpr int lm_tu(int nk) { return nk == 1 ? 4 : 2; }

template <int NK>
__global__ __launch_bounds__(64) void rq_log_metrics_k(LogMetricsArgs a)
{
    extern __shared__ __attribute__((aligned(16))) char lds_lm[];
    constexpr int NV = NK + 2;
    const int lane = lane_id();
    const int NS = a.log.n_sinks, NSTR = a.log.n_str;
    const int W = (NS + 31) >> 5, WS = (NSTR + 31) >> 5;
    double* scratch = reinterpret_cast<double*>(lds_lm);
    Cell* cell = reinterpret_cast<Cell*>(lds_lm + RQ_LM_SCRATCH_BYTES);
    uint32_t* sbits = reinterpret_cast<uint32_t*>(cell);   // step 1 only
    uint32_t* xbits = reinterpret_cast<uint32_t*>(lds_lm + RQ_LM_SCRATCH_BYTES + a.state_bytes);
    uint16_t* xpre = reinterpret_cast<uint16_t*>(xbits + W);

    // this block's rows
    char* slot = a.rows + (size_t)blockIdx.x * a.slot_bytes;
    double* Rt = reinterpret_cast<double*>(slot);
    double* Rs = Rt + a.log.ev_cap;
    uint32_t* Rv = reinterpret_cast<uint32_t*>(Rs + a.log.ev_cap);
    uint32_t* Rc = Rv + a.log.ev_cap;

    int64_t km1[NK];
#pragma unroll
    for (int q = 0; q < NK; ++q) km1[q] = (int64_t)a.Ks[q] - 1;

    for (int64_t r = blockIdx.x; r < a.log.n_rep; r += gridDim.x) {
        // ---- 1. the replica's pivot columns ----
        int64_t n = a.log.counts[r * 4 + 2];
        n = n < 0 ? 0 : (n > a.log.ev_cap ? a.log.ev_cap : n);
        const int32_t* J = a.log.ev_src + r * a.log.ev_cap;
        for (int w = lane; w < WS; w += 64) sbits[w] = 0u;
        for (int w = lane; w < W; w += 64) xbits[w] = 0u;
        wave_lds_sync();
        for (int64_t k0 = 0; k0 < n; k0 += 64) {
            const int64_t k = k0 + lane;
            if (k < n) {
                const int j = J[k];
                if ((unsigned)j < (unsigned)NSTR) atomicOr(&sbits[j >> 5], 1u << (j & 31));
            }
        }
        wave_lds_sync();
        for (int w0 = 0; w0 < WS; w0 += 64) {
            const uint32_t m = w0 + lane < WS ? sbits[w0 + lane] : 0u;
            uint64_t nz = __ballot(m != 0u);
            while (nz) {
                const int l = __ffsll((unsigned long long)nz) - 1;
                nz &= nz - 1;
                uint32_t mw = (uint32_t)bcast_i((int)m, l);
                while (mw) {
                    const int j = (w0 + l) * 32 + (__ffs(mw) - 1);
                    mw &= mw - 1;
                    const int p0 = a.log.csr_ptr[j], p1 = a.log.csr_ptr[j + 1];
                    for (int e = p0 + lane; e < p1; e += 64) {
                        const int x = a.log.csr_col[e];
                        atomicOr(&xbits[x >> 5], 1u << (x & 31));
                    }
                }
            }
        }
        wave_lds_sync();
        int S = 0;
        for (int w0 = 0; w0 < W; w0 += 64) {
            const int w = w0 + lane;
            const uint32_t c = w < W ? (uint32_t)__popc(xbits[w]) : 0u;
            const uint32_t inc = wave_scan_add(c);
            if (w < W) xpre[w] = (uint16_t)(S + (int)(inc - c));
            S += __builtin_amdgcn_readlane((int)inc, 63);
        }
        for (int c = lane; c < S; c += 64) {   // the stream bits are dead: every lane read its words
            Cell z;
            z.rank = -1;
            z.tag = -1;
            z.cs = 0;
            cell[c] = z;
        }
        wave_lds_sync();

        // ---- 2. the pivot rows ----
        int64_t sumI = 0;            // the sum of the integral cells
        int nvalid = 0, nfrac = 0;   // columns with a cell; with a fractional one
        int cK[NK];
#pragma unroll
        for (int q = 0; q < NK; ++q) cK[q] = 0;
        int gid = 0;
        bool have = false, tie = false;
        double pend_t = 0.0;         // the open t-group's time
        int64_t n_own = 0, n_oth = 0, nrow = 0;
        double r_t = 0.0, r_s = 0.0;   // lane (row & 63) stages a row
        int r_v = 0, r_c[NK];
#pragma unroll
        for (int q = 0; q < NK; ++q) r_c[q] = 0;

        auto store_row = [&](int64_t rr) {
            Rt[rr] = r_t;
            Rs[rr] = r_s;
            Rv[rr] = (uint32_t)r_v;
#pragma unroll
            for (int q = 0; q < NK; ++q) Rc[rr * NK + q] = (uint32_t)r_c[q];
        };
        auto emit = [&]() {   // the open group's pivot row
            double rowsum;
            if (nfrac == 0) {
                rowsum = (double)sumI;
            } else {
                double o[1];
                wave_npsum<1>((int64_t)S,
                              [&](int64_t k, double* v) {
                                  const Cell c = cell[k];
                                  v[0] = c.tag >= 0 ? (double)(int64_t)(c.cs >> 24) / (double)(int)(c.cs & 0xFFFFFFu)
                                                    : 0.0;
                              },
                              scratch, o);
                rowsum = o[0];
            }
            const int sl = (int)(nrow & 63);
            if (lane == sl) {
                r_t = pend_t;
                r_s = rowsum;
                r_v = nvalid;
#pragma unroll
                for (int q = 0; q < NK; ++q) r_c[q] = cK[q];
            }
            if (sl == 63) store_row(nrow - 63 + lane);
            ++nrow;
        };

        log_walk(a.log, r, [&](double t, bool own, int p0, int p1, int xfirst) {
            if (have && t != pend_t) {
                emit();
                ++gid;
            }
            have = true;
            pend_t = t;
            if (own) ++n_own;
            else ++n_oth;
            for (int e = p0; e < p1; e += 64) {
                const bool act = e + lane < p1;
                const int x = row_sink(a.log, e, p0, act, xfirst);
                bool ov = false, same = false;
                int64_t sm = 0, ns = 0;
                int k = 0, nk = 1;
                if (act) {
                    const uint32_t wb = xbits[x >> 5];
                    const int c = (int)xpre[x >> 5] + __popc(wb & ((1u << (x & 31)) - 1u));
                    Cell s = cell[c];
                    ov = s.tag >= 0;
                    same = s.tag == gid;
                    k = (int)(s.cs & 0xFFFFFFu);
                    sm = (int64_t)(s.cs >> 24);
                    const int rn = next_rank(own, s.rank);
                    nk = same ? k + 1 : 1;
                    ns = same ? sm + rn : (int64_t)rn;
                    s.rank = rn;
                    s.tag = gid;
                    s.cs = ((uint64_t)ns << 24) | (uint32_t)nk;
                    cell[c] = s;
                }
                if (__ballot(same)) tie = true;
                nvalid += popc(__ballot(act && !ov));
                // the old cell sm / k and the new one ns / nk
                const uint64_t means = __ballot(act && (nk > 1 || k > 1));
                if (!means) {   // both are the integers sm and ns
#pragma unroll
                    for (int q = 0; q < NK; ++q) {
                        const bool a1 = act && ns <= km1[q], a0 = ov && sm <= km1[q];
                        cK[q] += popc(__ballot(a1 && !a0)) - popc(__ballot(a0 && !a1));
                    }
                    // an own row: every new cell is 0; another's: old + 1, and 1 on a new column
                    if (own) sumI -= wave_sum_i64(ov ? sm : 0);
                    else sumI += popc(__ballot(act));
                } else {
                    // a quotient of integers < 2^53 is exact when it is an integer, so
                    // trunc(q) * den == num holds for an integral cell and for no other
                    const int kk = k > 0 ? k : 1;
                    const int64_t oq = (int64_t)((double)sm / (double)kk);
                    const int64_t nq = (int64_t)((double)ns / (double)nk);
                    const bool oint = ov && oq * kk == sm;
                    const bool ofr = ov && !oint;
                    const bool nint = nq * nk == ns;
                    nfrac += popc(__ballot(act && !nint && !ofr)) - popc(__ballot(act && nint && ofr));
#pragma unroll
                    for (int q = 0; q < NK; ++q) {
                        const bool a1 = act && ns <= km1[q] * nk, a0 = ov && sm <= km1[q] * kk;
                        cK[q] += popc(__ballot(a1 && !a0)) - popc(__ballot(a0 && !a1));
                    }
                    sumI += wave_sum_i64(act && nint ? nq : 0) - wave_sum_i64(oint ? oq : 0);
                }
            }
            wave_lds_sync();
        });
        if (have) emit();
        {   // the staged rows of the last, partial store
            const int rem = (int)(nrow & 63);
            if (lane < rem) store_row(nrow - rem + lane);
        }

        // ---- 3. counts, status and the integrals ----
        if (lane == 0) {
            int64_t* oc = a.out_counts + r * 4;
            oc[0] = n_own;
            oc[1] = n_oth;
            oc[2] = nrow;
            oc[3] = S;
            a.status[r] = log_status(have, tie);
        }
        double* M = a.metrics + r * NV;
        if (!have) {
            if (lane < NV) M[lane] = __builtin_nan("");
        } else {
            // every row was stored by this wave: drain its stores, then order them before
            // its loads at workgroup scope (same wave, same CU)
            __asm__ volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
            double res[NV];
            scan_rows<NK, lm_tu(NK), RQ_LM_NL>(nrow, (double)S, a.log.end, Rt, Rs, Rv, Rc, scratch, res);
            if (lane == 0) {
#pragma unroll
                for (int q = 0; q < NV; ++q) M[q] = res[q];
            }
        }
        wave_lds_sync();   // the scan's scratch and the cells before the next replica's marks
    }
}

template <int NK>
hipError_t launch_nk(const LogMetricsArgs& a, hipStream_t s)
{
    const size_t lds = rq_log_metrics_lds_bytes(a.log.n_sinks, a.log.n_str);
    hipLaunchKernelGGL((rq_log_metrics_k<NK>), dim3((unsigned)a.n_slots), dim3(64), lds, s, a);
    return hipGetLastError();
}

}  // namespace

hipError_t rq_launch_log_metrics(const LogMetricsArgs& a, hipStream_t s)
{
    switch (a.nK) {
    case 1: return launch_nk<1>(a, s);
    case 2: return launch_nk<2>(a, s);
    case 3: return launch_nk<3>(a, s);
    case 4: return launch_nk<4>(a, s);
    }
    return hipErrorInvalidValue;
}

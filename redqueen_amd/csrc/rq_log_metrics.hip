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
// rq_log_metrics_of (rq_log_metrics_of_k) plays the same steps for any tracked streams:
// steps 2 and 3 are one body, lm_play, instantiated for both kernels.  Its work items are
// (replica, tracked source); a block plays a contiguous range of them in its slot.  "Own"
// is the tracked stream (a LogView of the item with ctrl_idx = it).  Scope DF: step 1 does
// not depend on the source, so xbits / xpre / S are kept while the replica stays the same.
// Scope OWN: xbits is ANDed with the tracked stream's follower bits, built from its CSR row
// where the cells will be, and step 2 (MASKED) plays a sink only if its bit is set; an
// event none of whose sinks is set opens no t-group and is not counted.
//
// LDS (rq_log_metrics_lds_bytes): [scratch of wave_npsum<1> / scan_rows][Cell x n_sinks,
// during step 1 the stream bits][xbits][xpre].  A Cell is 16 bytes -- rank i32, tag i32,
// and sum << 24 | count in 64 bits (ev_cap <= 2^20: count <= 2^20, sum < 2^40) -- one
// ds_read_b128 and one ds_write_b128 per row.
//
// The slim entries (rq_log_metrics_slim, rq_log_metrics_of_slim) are the same body on an
// 8-byte SlimCell (rq_log_metrics_slim_lds_bytes: up to 19,400 sinks): every kernel and every
// step that touches a cell is a template over the cell type, CellIO<CELL> holds the two
// layouts' load and store, and the 64-bit halves the slim cells lack live in the slot's spill
// words behind its rows.
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

// The slim cell.  A group with one row of the column has count 1 and sum == rank, and a cell
// without a row count 0 and sum 0: only a column's second row in a t-group makes cs more than
// the rank says.  So the cell keeps a bit for that case and cs itself goes to the slot's spill
// word of the column, in the workspace.  Bits: rank -1 .. 2^20 (ev_cap <= 2^20 rows), a whole
// i32; tm bits 0..20: tag + 1 (tag -1 .. 2^20 - 1, so 0 .. 2^20), bit 31: multi, bits 21..30
// spare.  One ds_read_b64 and one ds_write_b64 per row.
struct __attribute__((aligned(8))) SlimCell {
    int rank;      // as Cell's
    uint32_t tm;   // (tag + 1) | multi << 31
};
static_assert(sizeof(SlimCell) == RQ_LM_SLIM_CELL_BYTES, "rq_log_metrics_slim_lds_bytes");
static_assert(RQ_LM_MAX_EV_CAP <= (1 << 20), "tag + 1 and the rank in 21 bits");
constexpr uint32_t SLIM_TAG_MASK = (1u << 21) - 1u, SLIM_MULTI = 1u << 31;

// What lm_play reads of a cell and writes back, for either layout: load gives the tag and
// rank and the group's cs; store the row's new rank, tag and cs (nk rows of the group).
template <class CELL>
struct CellIO;
template <>
struct CellIO<Cell> {
    static constexpr bool SLIM = false;
    static __device__ __forceinline__ Cell empty()
    {
        Cell z;
        z.rank = -1;
        z.tag = -1;
        z.cs = 0;
        return z;
    }
    static __device__ __forceinline__ void load(const Cell* cell, const uint64_t*, int c, int& rank, int& tag,
                                                uint64_t& cs)
    {
        const Cell s = cell[c];
        rank = s.rank;
        tag = s.tag;
        cs = s.cs;
    }
    static __device__ __forceinline__ void store(Cell* cell, uint64_t*, int c, int rank, int tag, uint64_t cs, int)
    {
        Cell s;
        s.rank = rank;
        s.tag = tag;
        s.cs = cs;
        cell[c] = s;
    }
};
template <>
struct CellIO<SlimCell> {
    static constexpr bool SLIM = true;
    static __device__ __forceinline__ SlimCell empty()
    {
        SlimCell z;
        z.rank = -1;
        z.tm = 0u;
        return z;
    }
    static __device__ __forceinline__ void load(const SlimCell* cell, const uint64_t* spill, int c, int& rank,
                                                int& tag, uint64_t& cs)
    {
        const SlimCell s = cell[c];
        rank = s.rank;
        tag = (int)(s.tm & SLIM_TAG_MASK) - 1;
        // one row: count 1, sum = rank; no row: 0
        cs = tag >= 0 ? ((uint64_t)(uint32_t)s.rank << 24) | 1u : 0u;
        if (s.tm & SLIM_MULTI) cs = spill[c];
    }
    static __device__ __forceinline__ void store(SlimCell* cell, uint64_t* spill, int c, int rank, int tag,
                                                 uint64_t cs, int nk)
    {
        SlimCell s;
        s.rank = rank;
        s.tm = (uint32_t)(tag + 1) | (nk > 1 ? SLIM_MULTI : 0u);
        cell[c] = s;
        if (nk > 1) spill[c] = cs;
    }
};

// rows per lane and trip of the scan (TU of wave_npsum_rows), as the fused sweep's fws_tu
constexpr int lm_tu(int nk) { return nk == 1 ? 4 : 2; }

// a block's wave: its LDS and its slot of the workspace
template <class CELL>
struct LmWave {
    double* scratch;
    CELL* cell;
    uint32_t* sbits;   // step 1 only, in the cells' place: the stream bits, then (scope OWN) the follower bits
    uint32_t* xbits;
    uint16_t* xpre;
    double *Rt, *Rs;
    uint32_t *Rv, *Rc;
    uint64_t* spill;   // slim cells only: cs of the columns with several rows in their last t-group
};

template <class CELL>
__device__ __forceinline__ LmWave<CELL> lm_wave(const LogMetricsArgs& a, char* lds)
{
    LmWave<CELL> w;
    const int W = (a.log.n_sinks + 31) >> 5;
    w.scratch = reinterpret_cast<double*>(lds);
    w.cell = reinterpret_cast<CELL*>(lds + RQ_LM_SCRATCH_BYTES);
    w.sbits = reinterpret_cast<uint32_t*>(w.cell);
    w.xbits = reinterpret_cast<uint32_t*>(lds + RQ_LM_SCRATCH_BYTES + a.state_bytes);
    w.xpre = reinterpret_cast<uint16_t*>(w.xbits + W);
    char* slot = a.rows + (size_t)blockIdx.x * a.slot_bytes;
    w.Rt = reinterpret_cast<double*>(slot);
    w.Rs = w.Rt + a.log.ev_cap;
    w.Rv = reinterpret_cast<uint32_t*>(w.Rs + a.log.ev_cap);
    w.Rc = w.Rv + a.log.ev_cap;
    w.spill = reinterpret_cast<uint64_t*>(slot + a.spill_off);
    return w;
}

// step 1, the marks: xbits = the sinks replica r's log reaches
template <class CELL>
__device__ __forceinline__ void lm_reached(const LogView& v, int64_t r, const LmWave<CELL>& w)
{
    const int lane = lane_id();
    const int NSTR = v.n_str;
    const int W = (v.n_sinks + 31) >> 5, WS = (NSTR + 31) >> 5;
    uint32_t* sbits = w.sbits;
    uint32_t* xbits = w.xbits;
    int64_t n = v.counts[r * 4 + 2];
    n = n < 0 ? 0 : (n > v.ev_cap ? v.ev_cap : n);
    const int32_t* J = v.ev_src + r * v.ev_cap;
    for (int q = lane; q < WS; q += 64) sbits[q] = 0u;
    for (int q = lane; q < W; q += 64) xbits[q] = 0u;
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
                const int p0 = v.csr_ptr[j], p1 = v.csr_ptr[j + 1];
                for (int e = p0 + lane; e < p1; e += 64) {
                    const int x = v.csr_col[e];
                    atomicOr(&xbits[x >> 5], 1u << (x & 31));
                }
            }
        }
    }
    wave_lds_sync();
}

// scope OWN: xbits &= the followers of stream c, whose bits are built from its CSR row where
// the stream bits were (every lane has read its words of them)
template <class CELL>
__device__ __forceinline__ void lm_own_columns(const LogView& v, int c, const LmWave<CELL>& w)
{
    const int lane = lane_id();
    const int W = (v.n_sinks + 31) >> 5;
    uint32_t* fbits = w.sbits;
    for (int q = lane; q < W; q += 64) fbits[q] = 0u;
    wave_lds_sync();
    const int p0 = v.csr_ptr[c], p1 = v.csr_ptr[c + 1];
    for (int e = p0 + lane; e < p1; e += 64) {
        const int x = v.csr_col[e];
        atomicOr(&fbits[x >> 5], 1u << (x & 31));
    }
    wave_lds_sync();
    for (int q = lane; q < W; q += 64) w.xbits[q] &= fbits[q];
    wave_lds_sync();
}

// step 1, the index: xpre of xbits; returns S
template <class CELL>
__device__ __forceinline__ int lm_index(const LogView& v, const LmWave<CELL>& w)
{
    const int lane = lane_id();
    const int W = (v.n_sinks + 31) >> 5;
    int S = 0;
    for (int w0 = 0; w0 < W; w0 += 64) {
        const int q = w0 + lane;
        const uint32_t c = q < W ? (uint32_t)__popc(w.xbits[q]) : 0u;
        const uint32_t inc = wave_scan_add(c);
        if (q < W) w.xpre[q] = (uint16_t)(S + (int)(inc - c));
        S += __builtin_amdgcn_readlane((int)inc, 63);
    }
    return S;
}

// S cells without a row (what step 1 kept in their place is dead: every lane read its words)
template <class CELL>
__device__ __forceinline__ void lm_cells(int S, const LmWave<CELL>& w)
{
    // (slim: a cleared cell has no multi bit, so the spill words a block's earlier replicas
    // left are never read and need no reset)
    for (int c = lane_id(); c < S; c += 64) w.cell[c] = CellIO<CELL>::empty();
    wave_lds_sync();
}

// Steps 2 and 3 of one replica for one tracked stream, log.ctrl_idx: the pivot rows of
// replica r over the S columns of xbits / xpre, then counts, status and the integrals to
// output element o.  MASKED (rq_log_metrics_of): a sink outside xbits gets no row, and an
// event none of whose sinks is a column is no event -- it opens no t-group and is not counted
// (xbits of rq_log_metrics holds every sink of every event, so there nothing is masked).
template <int NK, bool MASKED, class CELL>
__device__ __forceinline__ void lm_play(const LogMetricsArgs& a, const LogView& log, int64_t r, int64_t o, int S,
                                        const LmWave<CELL>& w, const int64_t (&km1)[NK])
{
    using IO = CellIO<CELL>;
    constexpr int NV = NK + 2;
    const int lane = lane_id();
    double* scratch = w.scratch;
    CELL* cell = w.cell;
    uint64_t* spill = w.spill;
    const uint32_t* xbits = w.xbits;
    const uint16_t* xpre = w.xpre;
    double *Rt = w.Rt, *Rs = w.Rs;
    uint32_t *Rv = w.Rv, *Rc = w.Rc;

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
            double o1[1];
            wave_npsum<1>((int64_t)S,
                          [&](int64_t k, double* v) {
                              int rk, tg;
                              uint64_t cs;
                              IO::load(cell, spill, (int)k, rk, tg, cs);
                              v[0] = tg >= 0 ? (double)(int64_t)(cs >> 24) / (double)(int)(cs & 0xFFFFFFu) : 0.0;
                          },
                          scratch, o1);
            rowsum = o1[0];
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
    auto open = [&](double t, bool own) {   // an event with a row joins the open t-group or closes it
        if (have && t != pend_t) {
            emit();
            ++gid;
        }
        have = true;
        pend_t = t;
        if (own) ++n_own;
        else ++n_oth;
    };

    log_walk(log, r, [&](double t, bool own, int p0, int p1, int xfirst) {
        bool opened = !MASKED;
        bool spilled = false;   // slim: a spill word was stored in this event
        if (!MASKED) open(t, own);
        for (int e = p0; e < p1; e += 64) {
            bool act = e + lane < p1;
            const int x = row_sink(log, e, p0, act, xfirst);
            bool ov = false, same = false;
            int64_t sm = 0, ns = 0;
            int k = 0, nk = 1;
            // the sink's word of the column bits and its prefix: both reads leave together,
            // before the mask is known, so masking adds no LDS round trip to an event
            uint32_t wb = 0u;
            int xp = 0;
            if (act) {
                wb = xbits[x >> 5];
                xp = (int)xpre[x >> 5];
            }
            if (MASKED) {
                act = act && ((wb >> (x & 31)) & 1u);
                if (!__ballot(act)) continue;
                if (!opened) open(t, own);
                opened = true;
            }
            if (act) {
                const int c = xp + __popc(wb & ((1u << (x & 31)) - 1u));
                int rk, tg;
                uint64_t cs;
                IO::load(cell, spill, c, rk, tg, cs);
                ov = tg >= 0;
                same = tg == gid;
                k = (int)(cs & 0xFFFFFFu);
                sm = (int64_t)(cs >> 24);
                const int rn = next_rank(own, rk);
                nk = same ? k + 1 : 1;
                ns = same ? sm + rn : (int64_t)rn;
                IO::store(cell, spill, c, rn, gid, ((uint64_t)ns << 24) | (uint32_t)nk, nk);
            }
            if (__ballot(same)) {   // same: nk > 1, the rows that store a spill word
                tie = true;
                spilled = true;
            }
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
        if (IO::SLIM && spilled) {
            // a spill word is loaded by whichever lane the column's next row falls on, in a
            // later event or in emit's sum: drain the stores and order them before those
            // loads at workgroup scope (same wave, same CU), as step 3 does for the rows.
            // The sinks of one row are distinct, so within the event nothing is re-read.
            __asm__ volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        }
    });
    if (have) emit();
    {   // the staged rows of the last, partial store
        const int rem = (int)(nrow & 63);
        if (lane < rem) store_row(nrow - rem + lane);
    }

    // ---- 3. counts, status and the integrals ----
    if (lane == 0) {
        int64_t* oc = a.out_counts + o * 4;
        oc[0] = n_own;
        oc[1] = n_oth;
        oc[2] = nrow;
        oc[3] = S;
        a.status[o] = log_status(have, tie);
    }
    double* M = a.metrics + o * NV;
    if (!have) {
        if (lane < NV) M[lane] = __builtin_nan("");
    } else {
        // every row was stored by this wave: drain its stores, then order them before
        // its loads at workgroup scope (same wave, same CU)
        __asm__ volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        double res[NV];
        scan_rows<NK, lm_tu(NK), RQ_LM_NL>(nrow, (double)S, log.end, Rt, Rs, Rv, Rc, scratch, res);
        if (lane == 0) {
#pragma unroll
            for (int q = 0; q < NV; ++q) M[q] = res[q];
        }
    }
    wave_lds_sync();   // the scan's scratch and the cells before the next marks
}

template <int NK, class CELL>
__global__ __launch_bounds__(64) void rq_log_metrics_k(LogMetricsArgs a)
{
    extern __shared__ __attribute__((aligned(16))) char lds_lm[];
    const LmWave<CELL> w = lm_wave<CELL>(a, lds_lm);
    int64_t km1[NK];
#pragma unroll
    for (int q = 0; q < NK; ++q) km1[q] = (int64_t)a.Ks[q] - 1;

    for (int64_t r = blockIdx.x; r < a.log.n_rep; r += gridDim.x) {
        lm_reached(a.log, r, w);
        const int S = lm_index(a.log, w);
        lm_cells(S, w);
        lm_play<NK, false>(a, a.log, r, r, S, w, km1);
    }
}

// The first work item of block b of B.  taper 1: equal shares.  taper a in (1, 2], for
// launches of more blocks than the device holds at once: shares falling linearly from a to
// 2 - a times the mean.  The device starts blocks in index order as earlier ones end, so the
// long ones go first and the short ones fill the tail, where equal shares leave most of the
// device idle in the last round (C3, 17 players, 943 -> 792 ms).
__device__ __forceinline__ int64_t of_first_item(int64_t n, unsigned b, unsigned B, double taper)
{
    if (taper > 1.0 && n >= 4 * (int64_t)B) {
        const double u = (double)b / (double)B;
        return b >= B ? n : (int64_t)((double)n * (u * (taper - (taper - 1.0) * u)));
    }
    return n * b / B;
}

// rq_log_metrics_of: block b plays the work items [n b / B, n (b + 1) / B) of the n = n_rep *
// n_src items (replica, tracked source), item = replica * n_src + position in src_ids -- for
// each replica it meets a run of consecutive tracked sources, played one after the other in
// the block's slot.  Scope DF: the columns are the replica's, found once per run.  Scope OWN:
// they are masked with the tracked source's followers, found again per source.
template <int NK, class CELL>
__global__ __launch_bounds__(64) void rq_log_metrics_of_k(LogMetricsOfArgs b)
{
    extern __shared__ __attribute__((aligned(16))) char lds_lm[];
    const LogMetricsArgs& a = b.m;
    const LmWave<CELL> w = lm_wave<CELL>(a, lds_lm);
    int64_t km1[NK];
#pragma unroll
    for (int q = 0; q < NK; ++q) km1[q] = (int64_t)a.Ks[q] - 1;

    const int64_t n_items = a.log.n_rep * b.n_src;
    const int64_t lo = of_first_item(n_items, blockIdx.x, gridDim.x, b.taper);
    const int64_t hi = of_first_item(n_items, blockIdx.x + 1, gridDim.x, b.taper);
    int64_t r_cols = -1;   // scope DF: the replica whose columns xbits / xpre hold
    int S = 0;
    for (int64_t it = lo; it < hi; ++it) {
        const int64_t r = it / b.n_src;
        const int k = (int)(it - r * b.n_src);
        LogView v = a.log;
        v.ctrl_idx = b.trk[k];
        if (b.scope == RQ_LOG_OF_OWN || r != r_cols) {
            lm_reached(v, r, w);
            if (b.scope == RQ_LOG_OF_OWN) lm_own_columns(v, v.ctrl_idx, w);
            S = lm_index(v, w);
            r_cols = r;
        }
        lm_cells(S, w);
        lm_play<NK, true>(a, v, r, it, S, w, km1);
    }
}

// the block's LDS: the cells' layout is the one the host sized state_bytes for
template <class CELL>
size_t lm_lds_bytes(const LogMetricsArgs& a)
{
    return CellIO<CELL>::SLIM ? rq_log_metrics_slim_lds_bytes(a.log.n_sinks, a.log.n_str)
                              : rq_log_metrics_lds_bytes(a.log.n_sinks, a.log.n_str);
}

template <int NK, class CELL>
hipError_t launch_nk(const LogMetricsArgs& a, hipStream_t s)
{
    const size_t lds = lm_lds_bytes<CELL>(a);
    hipLaunchKernelGGL((rq_log_metrics_k<NK, CELL>), dim3((unsigned)a.n_slots), dim3(64), lds, s, a);
    return hipGetLastError();
}

template <int NK, class CELL>
hipError_t launch_of_nk(LogMetricsOfArgs b, hipStream_t s)
{
    const size_t lds = lm_lds_bytes<CELL>(b.m);
    // tapered shares only when the blocks run in several rounds: with every block resident
    // the longest block is the launch's time
    const int64_t resident = (int64_t)rq_occupancy(rq_log_metrics_of_k<NK, CELL>, 64, lds) * rq_cu_count();
    b.taper = resident > 0 && b.m.n_slots > resident ? RQ_LM_OF_TAPER : 1.0;
    hipLaunchKernelGGL((rq_log_metrics_of_k<NK, CELL>), dim3((unsigned)b.m.n_slots), dim3(64), lds, s, b);
    return hipGetLastError();
}

template <class CELL>
hipError_t launch_cells(const LogMetricsArgs& a, hipStream_t s)
{
    switch (a.nK) {
    case 1: return launch_nk<1, CELL>(a, s);
    case 2: return launch_nk<2, CELL>(a, s);
    case 3: return launch_nk<3, CELL>(a, s);
    case 4: return launch_nk<4, CELL>(a, s);
    }
    return hipErrorInvalidValue;
}

template <class CELL>
hipError_t launch_of_cells(const LogMetricsOfArgs& b, hipStream_t s)
{
    switch (b.m.nK) {
    case 1: return launch_of_nk<1, CELL>(b, s);
    case 2: return launch_of_nk<2, CELL>(b, s);
    case 3: return launch_of_nk<3, CELL>(b, s);
    case 4: return launch_of_nk<4, CELL>(b, s);
    }
    return hipErrorInvalidValue;
}

}  // namespace

hipError_t rq_launch_log_metrics(const LogMetricsArgs& a, hipStream_t s, bool slim)
{
    return slim ? launch_cells<SlimCell>(a, s) : launch_cells<Cell>(a, s);
}

hipError_t rq_launch_log_metrics_of(const LogMetricsOfArgs& b, hipStream_t s, bool slim)
{
    return slim ? launch_of_cells<SlimCell>(b, s) : launch_of_cells<Cell>(b, s);
}

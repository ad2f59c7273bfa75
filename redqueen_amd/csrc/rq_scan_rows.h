// rq_scan_rows.h -- the numpy-order integrals over one replica's pivot rows (time_in_top_k
// utils.py:84-98, average_rank :101-114, int_r_2), by ONE wavefront: the one definition of
// the row, its loads and its integrands, shared by rq_scan (rq_kernels.hip) and by the
// merged fused sweep's epilogue (rq_sweep_fw.hip), so both give the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rq_device.h"

#pragma clang fp contract(off)

namespace rq {

// a pivot row as the scan holds it: from the four row arrays ...
template <int NK>
struct ScanRow {
    double t, s;
    uint32_t v, c[NK];
    __device__ __forceinline__ double sum() const { return s; }
    __device__ __forceinline__ uint32_t valid() const { return v; }
    __device__ __forceinline__ uint32_t cnt(int q) const { return c[q]; }
};
// ... or a 16-byte record of the merged fused sweep (RowStage<1, true>, rq_sweep_core.h), kept
// packed until it is used: four registers a row.  (double)(uint32) of the integer rank sum is
// the double the array layout stores, so the integrands get the same operands.
struct ScanRow16 {
    double t;
    uint32_t su, cv;
    __device__ __forceinline__ double sum() const { return (double)su; }
    __device__ __forceinline__ uint32_t valid() const { return cv >> 16; }
    __device__ __forceinline__ uint32_t cnt(int) const { return cv & 0xFFFFu; }
};

// the integrands of a row up to the next row's time t1, and the sums over rows [0, n)
template <int NK, int TU, int NL, class Row, class LD, class TLD>
__device__ __forceinline__ void scan_rows_of(int64_t n, double S, double end, LD&& ld, TLD&& tld, double* lds,
                                             double res[NK + 2])
{
    constexpr int NV = NK + 2;
    auto vf = [&](const Row& r, double t1, double* v) {
        const double dt = t1 - r.t;
        const double m = r.sum() / (double)r.valid();
#pragma unroll
        for (int q = 0; q < NK; ++q) v[q] = ((double)r.cnt(q) / S) * dt;
        v[NK] = m * dt;
        v[NK + 1] = (m * m) * dt;
    };
    wave_npsum_rows<NV, true, Row, TU, NL>(n, end, ld, tld, vf, lds, res);
}

// Rows [0, n) of a replica (n > 0) at Rt / Rs / Rv / Rc (Rc: NK counts per row), S its sink
// columns, end the horizon.  res[0..NK): time in the top K_q; res[NK]: average rank;
// res[NK + 1]: the integral of rank^2 -- in every lane.
// TU: rows per lane and trip (wave_npsum_rows); NL: the leaf capacity of the LDS layout,
// lds >= npsum_lds_doubles<NK + 2, NL>() doubles private to this wave.
template <int NK, int TU, int NL = 128>
__device__ __forceinline__ void scan_rows(int64_t n, double S, double end, const double* Rt, const double* Rs,
                                          const uint32_t* Rv, const uint32_t* Rc, double* lds,
                                          double res[NK + 2])
{
    using Row = ScanRow<NK>;
    auto ld = [&](uint32_t kk) {
        Row r;
        r.t = Rt[kk];
        r.s = Rs[kk];
        r.v = Rv[kk];
#pragma unroll
        for (int q = 0; q < NK; ++q) r.c[q] = Rc[kk * NK + q];
        return r;
    };
    auto tld = [&](uint32_t kk) { return Rt[kk]; };
    scan_rows_of<NK, TU, NL, Row>(n, S, end, ld, tld, lds, res);
}

// the same over 16-byte records R[0, n) (K = 1): one 16-byte load per row
template <int TU, int NL = 128>
__device__ __forceinline__ void scan_rows16(int64_t n, double S, double end, const uint4* R, double* lds,
                                            double res[3])
{
    auto ld = [&](uint32_t kk) {
        const uint4 x = R[kk];
        ScanRow16 r;
        r.t = rq_bits_dbl(((uint64_t)x.y << 32) | x.x);
        r.su = x.z;
        r.cv = x.w;
        return r;
    };
    auto tld = [&](uint32_t kk) { return reinterpret_cast<const double*>(R + kk)[0]; };
    scan_rows_of<1, TU, NL, ScanRow16>(n, S, end, ld, tld, lds, res);
}

}  // namespace rq

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
    constexpr int NV = NK + 2;
    struct Row {
        double t, s;
        uint32_t v, c[NK];
    };
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
    auto vf = [&](const Row& r, double t1, double* v) {
        const double dt = t1 - r.t;
        const double m = r.s / (double)r.v;
#pragma unroll
        for (int q = 0; q < NK; ++q) v[q] = ((double)r.c[q] / S) * dt;
        v[NK] = m * dt;
        v[NK + 1] = (m * m) * dt;
    };
    wave_npsum_rows<NV, true, Row, TU, NL>(n, end, ld, tld, vf, lds, res);
}

}  // namespace rq

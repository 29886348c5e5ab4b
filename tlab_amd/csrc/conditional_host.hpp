// Conditional statistics (conditional.hip, conditional.cpp): what the kernels and the host loops share -- the level of a point (FI_GATE,
// mappings/fi_gate.f90:65-90), the integer power of the gated moments (AVG1V2D / AVG1V2D1G, utils/averages.f90:114-137, :172-209), RAW_TO_CENTRAL
// (statistics/avg_xz.f90:72-102) -- and the constants a test mirrors.  The bin of a point is pdf_bin of pdfs_host.hpp, unchanged: a value goes
// to the bin its count goes to.
#pragma once
#include <hip/hip_runtime.h>

#include "pdfs_host.hpp"

#pragma clang fp contract(off)      // every operation below stays as written

namespace tlab {

constexpr int CAVG_MAX_BINS = 1024;            // nbins of tlab_cavg1v_n, nbins(1)*nbins(2) of tlab_cavg2v: above it TLAB_EINVAL
constexpr int CAVG_WAVES = 4;                  // waves of a workgroup of k_cavg_sum; each owns a table of its own
constexpr int CAVG_LDS_BYTES = 49152;          // sums and counts of one workgroup: waves x tables x nbins x columns x (8 + 4) bytes
constexpr int COND_MAX_MOMENTS = 10;           // NMOMS_MAX of statistics/avg_xz.f90
constexpr int COND_LEVELS_PER_LAUNCH = 4;      // gate levels whose sums one launch of k_gated_moments keeps in registers (no scratch: DESIGN.md 7)
constexpr int GATE_MAX_THRESHOLDS = GATE_MAX_LEVELS - 1;

// Columns of a wave's table: the largest power of two <= 64 with which ntab tables of nbins bins fit CAVG_LDS_BYTES; 0: not even one
inline int cavg_columns(int nbins, int ntab) {
    int cols = 64;
    while (cols >= 1 && (long long)CAVG_WAVES * ntab * nbins * cols * 12 > CAVG_LDS_BYTES) cols >>= 1;
    return cols;
}

// fi_gate.f90:85-90: the first n in 1 .. igate_size - 1 with a < thr(n), else igate_size (thresholds ascending; a NaN gets igate_size)
__host__ __device__ __forceinline__ signed char gate_level(double a, const double *thr, int igate_size) {
    int n = 1;
    for (; n < igate_size; ++n)
        if (a < thr[n - 1]) break;
    return (signed char)n;
}

// fi_gate.f90:65-71: the quadrants of (a, v), with exactly its comparisons
__host__ __device__ __forceinline__ signed char gate_quadrant(double a, double v) {
    if (a > 0.0 && v >= 0.0) return 1;
    if (a <= 0.0 && v > 0.0) return 2;
    if (a < 0.0 && v <= 0.0) return 3;
    return 4;
}

// x**m for a run-time integer m >= 0 as the Fortran runtime forms it: square and multiply from the low bit
inline double ipow(double x, int m) {
    double r = 1.0;
    for (unsigned b = (unsigned)m;;) {
        if (b & 1u) r *= x;
        b >>= 1;
        if (!b) break;
        x *= x;
    }
    return r;
}

// x**1 .. x**NM with the very products ipow forms: p[m - 1] = x**m
template <int NM>
__host__ __device__ __forceinline__ void powers(double a, double *p) {
    const double a2 = a * a, a4 = a2 * a2, a8 = a4 * a4, a3 = a * a2;
    const double all[COND_MAX_MOMENTS] = {a, a2, a3, a4, a * a4, a2 * a4, a3 * a4, a8, a * a8, a2 * a8};
#pragma unroll
    for (int m = 0; m < NM; ++m) p[m] = all[m];
}

// RAW_TO_CENTRAL (avg_xz.f90:72-102): moments(1 .. nm) in place, left to right as written there
inline void raw_to_central(int nm, double *moments) {
    double aux[COND_MAX_MOMENTS];
    for (int i = 0; i < nm; ++i) aux[i] = moments[i];
    for (int im = 2; im <= nm; ++im) {
        moments[im - 1] = 0.0;
        for (int k = 0; k <= im - 1; ++k) {
            double num = 1.0, den = 1.0;
            for (int i = im; i >= im - k + 1; --i) num = num * (double)i;
            for (int i = k; i >= 1; --i) den = den * (double)i;
            moments[im - 1] = moments[im - 1] + num / den * aux[im - k - 1] * ipow(-aux[0], k);
        }
        moments[im - 1] = moments[im - 1] + ipow(-aux[0], im);
    }
}

}  // namespace tlab

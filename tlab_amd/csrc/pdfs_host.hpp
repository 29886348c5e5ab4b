// Plane PDFs (pdfs.hip, pdfs.cpp): what the kernels and the host loop share -- the bin of a point, the interval of a histogram, PDF_ANALIZE -- and
// the constants a test mirrors.  Module PDFS of the reference (utils/pdfs.f90) and PDF1V_N / PDF2V (statistics/pdf.f90).
//
// The bin of a point is up = int(q) + 1 with q = (u - umin)/ustep: one subtraction and one division in fp64, unfused (the pragma below: this header
// is code of both sides).  Fortran's int() truncates toward zero, so with an external interval a value slightly below umin (q in (-1, 0)) is
// counted in bin 1 and a value equal to umax (q = nbins) is dropped; both are reproduced.  Where int() is undefined (q outside the integers, NaN)
// the result is DEFINED here so that no index leaves the table: an external interval counts a point iff -1 < q < nbins; a local interval (the
// last point goes to the last bin, up = min(up, nbins)) counts every finite q > -1.  NaN and infinities are dropped.  Fields that hold NaN are
// outside the contract: min / max of them are not the reference's.
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>

#pragma clang fp contract(off)      // every operation below stays as written

namespace tlab {

constexpr int PDF_ROWS_PER_GROUP = 32;      // rows of k one workgroup of k_pdf_minmax / k_pdf_hist takes (tests/test_gpu_pdfs.py mirrors it)
constexpr int PDF_MAX_BINS = 4096;          // nbins of tlab_pdf1v_n, nbins(1)*nbins(2) of tlab_pdf2v: above it TLAB_EINVAL
constexpr int PDF_LDS_WORDS = 8192;         // 32-bit counters of one workgroup: 2 tables (plane, volume) x nbins x replicas
constexpr int PDF_FIELDS_PER_LAUNCH = 8;    // more fields go in groups
constexpr int GATE_MAX_LEVELS = 127;        // np of tlab_inter_n_xz: the positive values of an int8 gate
constexpr double PDF_BIG = 1.0e20;         // big_wp (base/tlab_constants.f90): where the gated min / max start

// the 0-based bin of u, or -1 for a point that is not counted
__host__ __device__ __forceinline__ int pdf_bin(double u, double umin, double ustep, int nbins, bool ext) {
    const double q = (u - umin) / ustep;
    if (!(q > -1.0)) return -1;                            // (NaN fails every comparison)
    if (q < (double)nbins) return (int)q;                  // q in (-1, nbins): trunc(q) in [0, nbins - 1]
    return (!ext && q <= DBL_MAX) ? nbins - 1 : -1;
}

// utils/pdfs.f90:68-71: the step of [umin, umax] in nbins bins, the centres of the first and the last bin (what pdf(nbins+1), pdf(nbins+2) hold),
// and only then the replacement of a zero step
inline double pdf_step(double umin, double umax, int nbins, double *first, double *last) {
    double ustep = (umax - umin) / (double)nbins;
    *first = umin + 0.5 * ustep;
    *last = umax - 0.5 * ustep;
    if (ustep == 0.0) ustep = 1.0;
    return ustep;
}

// PDF_ANALIZE (utils/pdfs.f90:329-379): pdf = nbins counts and the two centres; maxval of an empty range is -huge, as in Fortran
inline void pdf_analize(int ibc, int nbins, const double *pdf, double *umin_ext, double *umax_ext, double plim, int *nplim) {
    const double first = pdf[nbins], ustep = (pdf[nbins + 1] - pdf[nbins]) / (double)(nbins - 1);
    int upmin = 1, upmax = nbins;
    if (ibc == 1 || ibc == 3) upmin = upmin + 1;
    if (ibc == 2 || ibc == 3) upmax = upmax - 1;
    *umin_ext = first - 0.5 * ustep + ustep * (double)(upmin - 1);
    *umax_ext = first - 0.5 * ustep + ustep * (double)upmax;
    double mx = -DBL_MAX;
    for (int up = upmin; up <= upmax; ++up) mx = pdf[up - 1] > mx ? pdf[up - 1] : mx;
    const double threshold = plim * mx;
    *nplim = 0;
    for (int up = upmin; up <= upmax; ++up)
        if (pdf[up - 1] > threshold) *nplim = *nplim + 1;
    for (int up = upmin; up <= upmax; ++up)
        if (pdf[up - 1] > threshold) {
            *umin_ext = first - 0.5 * ustep + ustep * (double)(up - 1);
            break;
        }
    for (int up = upmax; up >= upmin; --up)
        if (pdf[up - 1] > threshold) {
            *umax_ext = first - 0.5 * ustep + ustep * (double)up;
            break;
        }
}

}  // namespace tlab

// The monitors of the main loop on the device (monitor.hip): TIME_COURANT's maximum and DNS_BOUNDS_CONTROL's extremes with their location.
// Each call runs on stream st and returns host values (it synchronises the stream).
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

namespace tlab {
// pmax = max over the box (nx, ny, nz) of |u| odx(i + ioff) + |v| ody(j) [+ |w| odz(k + koff) if zon]  (time.f90:395-454); odx, odz: GLOBAL tables
hipError_t monitor_courant_max(const double *u, const double *v, const double *w, const double *odx, const double *ody, const double *odz, int nx, int ny,
                               int nz, int ioff, int koff, int zon, double *pmax, hipStream_t st);
// min / max of a[i] (+ b[i] if b) over i < n and the first 0-based flat index of each (imn, imx may be NULL)
hipError_t monitor_extremes(const double *a, const double *b, long long n, double *mn, double *mx, long long *imn, long long *imx, hipStream_t st);

// The location of an extreme across ranks without a MAXLOC operation: val[l] (the extreme of local rank l) and gidx[l] (its global column-major
// index) of the local ranks; allreduce(values, n, op) is the transport's (op 0 = MPI_MAX, 1 = MPI_MIN, in place over values[l * n]).  The value is
// all-reduced first, then the smallest index among the ranks that hold it.  On return val[0], gidx[0] are the global result.
template <class AR>
int monitor_allreduce_extreme(AR allreduce, int op, std::vector<double> &val, std::vector<double> &gidx) {
    const std::vector<double> mine = val;
    int rc = allreduce(val.data(), 1, op);
    if (rc < 0) return rc;
    for (size_t l = 0; l < val.size(); ++l) gidx[l] = mine[l] == val[l] ? gidx[l] : 1.0e300;      // (indices < 2^53: exact as doubles)
    return allreduce(gidx.data(), 1, 1);
}
// 1-based (i, j, k) of a global column-major index of an (nx, ny, *) box
inline void monitor_ijk(double g, int nx, int ny, int *ijk) {
    if (!ijk) return;
    const long long e = (long long)g;
    ijk[0] = (int)(e % nx) + 1; ijk[1] = (int)((e / nx) % ny) + 1; ijk[2] = (int)(e / ((long long)nx * ny)) + 1;
}
}  // namespace tlab

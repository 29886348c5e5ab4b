// Per-iteration monitors of the main loop on the device (tools/dns/dns_main.f90:268, :273):
//   TIME_COURANT (tools/dns/time.f90:395-454, incompressible): max over the box of |u| odx(i + ioff) + |v| ody(j) + |w| odz(k + koff)
//   DNS_BOUNDS_CONTROL (tools/dns/dns_local.f90:157-230): min / max of the divergence with the first column-major index of each (minloc / maxloc)
// Both are two-stage deterministic reductions: per wave by shuffles, per block through LDS, the block partials to HBM, one small final block.
// No atomics: the result is a function of the data alone.  The final values travel back with one copy and a synchronisation of the stream.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstdint>

#include "monitor.hpp"
#include "profile.hpp"

namespace tlab {
namespace {

constexpr int MON_THREADS = 256, MON_WAVES = MON_THREADS / 64, MON_MAX_GRID = 2048;

// ---- Courant number: max of |u| odx + |v| ody (+ |w| odz), one line of nx points per row -------------------------------------------------------
// The box is walked as lines (j, k): j and k come from one division per line, i from the position in the line.  V = 2: 16-B loads (nx even,
// arrays 16-B aligned); V = 1: scalar loads.  A block takes `rows` lines at once when a line has fewer vectors than the block has threads.
template <int V>
__global__ void __launch_bounds__(MON_THREADS) k_courant_partial(const double *__restrict__ u, const double *__restrict__ v, const double *__restrict__ w,
                                                                 const double *__restrict__ odx, const double *__restrict__ ody,
                                                                 const double *__restrict__ odz, int nx, int ny, int nlines, int ioff, int koff,
                                                                 int zon, double *__restrict__ part) {
    __shared__ double smx[MON_WAVES];
    const int L = nx / V;
    const int rows = L >= MON_THREADS ? 1 : MON_THREADS / L;
    const int r = L >= MON_THREADS ? 0 : (int)threadIdx.x / L;
    const int x0 = L >= MON_THREADS ? (int)threadIdx.x : (int)threadIdx.x % L;
    const int xs = L >= MON_THREADS ? MON_THREADS : L;
    double mx = -1.0e300;
    if (r < rows) {
        for (int line = (int)blockIdx.x * rows + r; line < nlines; line += (int)gridDim.x * rows) {
            const int j = line % ny, k = line / ny;
            const double oy = ody[j], oz = zon ? odz[k + koff] : 0.0;
            const size_t base = (size_t)line * nx;
            for (int xv = x0; xv < L; xv += xs) {
                const int i = xv * V;
                if constexpr (V == 2) {
                    const double2 a = *reinterpret_cast<const double2 *>(u + base + i);
                    const double2 b = *reinterpret_cast<const double2 *>(v + base + i);
                    double v0 = fabs(a.x) * odx[i + ioff] + fabs(b.x) * oy;
                    double v1 = fabs(a.y) * odx[i + 1 + ioff] + fabs(b.y) * oy;
                    if (zon) {      // the GLOBAL z%size > 1 (time.f90:402), not the depth of the rank
                        const double2 c = *reinterpret_cast<const double2 *>(w + base + i);
                        v0 += fabs(c.x) * oz;
                        v1 += fabs(c.y) * oz;
                    }
                    mx = fmax(mx, fmax(v0, v1));
                } else {
                    double v0 = fabs(u[base + i]) * odx[i + ioff] + fabs(v[base + i]) * oy;
                    if (zon) v0 += fabs(w[base + i]) * oz;
                    mx = fmax(mx, v0);
                }
            }
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) mx = fmax(mx, __shfl_xor(mx, d, 64));
    if ((threadIdx.x & 63) == 0) smx[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
        double m = smx[0];
        for (int i = 1; i < MON_WAVES; ++i) m = fmax(m, smx[i]);
        part[blockIdx.x] = m;
    }
}

__global__ void __launch_bounds__(MON_THREADS) k_courant_final(const double *__restrict__ part, int np, double *__restrict__ out) {
    __shared__ double smx[MON_WAVES];
    double mx = -1.0e300;
    for (int i = threadIdx.x; i < np; i += MON_THREADS) mx = fmax(mx, part[i]);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) mx = fmax(mx, __shfl_xor(mx, d, 64));
    if ((threadIdx.x & 63) == 0) smx[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
        double m = smx[0];
        for (int i = 1; i < MON_WAVES; ++i) m = fmax(m, smx[i]);
        out[0] = m;
    }
}

// ---- extremes with their first location: minval / maxval + minloc / maxloc of a (+ b) ----------------------------------------------------------
// (value, index) pairs are ordered by value, then by index: the smaller index wins a tie in both directions, as the first occurrence of Fortran's
// minloc / maxloc.  NaN compares false everywhere and never becomes an extreme.
struct Ext {
    double mn, mx;
    long long imn, imx;
};
__device__ __forceinline__ void ext_take(Ext &e, double x, long long i) {
    if (x < e.mn || (x == e.mn && i < e.imn)) { e.mn = x; e.imn = i; }
    if (x > e.mx || (x == e.mx && i < e.imx)) { e.mx = x; e.imx = i; }
}
__device__ __forceinline__ void ext_merge(Ext &e, const Ext &o) {
    if (o.mn < e.mn || (o.mn == e.mn && o.imn < e.imn)) { e.mn = o.mn; e.imn = o.imn; }
    if (o.mx > e.mx || (o.mx == e.mx && o.imx < e.imx)) { e.mx = o.mx; e.imx = o.imx; }
}
__device__ __forceinline__ Ext ext_none() { return Ext{INFINITY, -INFINITY, LLONG_MAX, LLONG_MAX}; }
// per-wave then per-block; thread 0 holds the block's result
__device__ __forceinline__ Ext ext_block(Ext e) {
    __shared__ Ext s[MON_WAVES];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        Ext o;
        o.mn = __shfl_xor(e.mn, d, 64); o.imn = __shfl_xor(e.imn, d, 64);
        o.mx = __shfl_xor(e.mx, d, 64); o.imx = __shfl_xor(e.imx, d, 64);
        ext_merge(e, o);
    }
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = e;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int i = 1; i < MON_WAVES; ++i) ext_merge(e, s[i]);
    return e;
}

// part: values [2][gridDim.x] (min, max), indices [2][gridDim.x] behind them.  V = 2: 16-B loads (n even, arrays 16-B aligned).
template <int V, bool TWO>
__global__ void __launch_bounds__(MON_THREADS) k_extremes_partial(const double *__restrict__ a, const double *__restrict__ b, long long n,
                                                                  double *__restrict__ pv, long long *__restrict__ pi) {
    Ext e = ext_none();
    const long long nv = n / V, stride = (long long)gridDim.x * MON_THREADS;
    for (long long t = (long long)blockIdx.x * MON_THREADS + threadIdx.x; t < nv; t += stride) {
        if constexpr (V == 2) {
            double2 x = *reinterpret_cast<const double2 *>(a + 2 * t);
            if constexpr (TWO) {
                const double2 y = *reinterpret_cast<const double2 *>(b + 2 * t);
                x.x += y.x; x.y += y.y;
            }
            ext_take(e, x.x, 2 * t);
            ext_take(e, x.y, 2 * t + 1);
        } else {
            double x = a[t];
            if constexpr (TWO) x += b[t];
            ext_take(e, x, t);
        }
    }
    e = ext_block(e);
    if (threadIdx.x == 0) {
        pv[blockIdx.x] = e.mn; pv[gridDim.x + blockIdx.x] = e.mx;
        pi[blockIdx.x] = e.imn; pi[gridDim.x + blockIdx.x] = e.imx;
    }
}

// out: mn, mx, then the two indices as 64-bit integers in the next two slots
__global__ void __launch_bounds__(MON_THREADS) k_extremes_final(const double *__restrict__ pv, const long long *__restrict__ pi, int np,
                                                                double *__restrict__ out) {
    Ext e = ext_none();
    for (int i = threadIdx.x; i < np; i += MON_THREADS) {
        const Ext o{pv[i], pv[np + i], pi[i], pi[np + i]};
        ext_merge(e, o);
    }
    e = ext_block(e);
    if (threadIdx.x == 0) {
        out[0] = e.mn; out[1] = e.mx;
        reinterpret_cast<long long *>(out)[2] = e.imn;
        reinterpret_cast<long long *>(out)[3] = e.imx;
    }
}

// block partials and the final result: one buffer for the process (the monitors run on the library's stream one after the other)
double *scratch() {
    static double *p = nullptr;
    if (!p && hipMalloc((void **)&p, (size_t)(4 * MON_MAX_GRID + 8) * sizeof(double)) != hipSuccess) p = nullptr;
    return p;
}
bool aligned16(const void *p) { return p == nullptr || ((uintptr_t)p & 15) == 0; }

}  // namespace

hipError_t monitor_courant_max(const double *u, const double *v, const double *w, const double *odx, const double *ody, const double *odz, int nx, int ny,
                               int nz, int ioff, int koff, int zon, double *pmax, hipStream_t st) {
    double *buf = scratch();
    if (!buf) return hipErrorOutOfMemory;
    if (nx < 1 || ny < 1 || nz < 1) return hipErrorInvalidValue;
    const int nlines = ny * nz;
    const bool vec = nx % 2 == 0 && aligned16(u) && aligned16(v) && (!zon || aligned16(w));
    const int L = vec ? nx / 2 : nx, rows = L >= MON_THREADS ? 1 : MON_THREADS / L;
    const int grid = std::max(1, std::min(MON_MAX_GRID, (nlines + rows - 1) / rows));
    double *res = buf + 4 * MON_MAX_GRID;
    {
        ProfScope ps("k_courant_partial", st, (double)nx * nlines * (zon ? 24.0 : 16.0));
        if (vec) hipLaunchKernelGGL(k_courant_partial<2>, dim3(grid), dim3(MON_THREADS), 0, st, u, v, w, odx, ody, odz, nx, ny, nlines, ioff, koff, zon, buf);
        else hipLaunchKernelGGL(k_courant_partial<1>, dim3(grid), dim3(MON_THREADS), 0, st, u, v, w, odx, ody, odz, nx, ny, nlines, ioff, koff, zon, buf);
    }
    hipLaunchKernelGGL(k_courant_final, dim3(1), dim3(MON_THREADS), 0, st, buf, grid, res);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if ((e = hipMemcpyAsync(pmax, res, sizeof(double), hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
    return hipStreamSynchronize(st);
}

hipError_t monitor_extremes(const double *a, const double *b, long long n, double *mn, double *mx, long long *imn, long long *imx, hipStream_t st) {
    double *buf = scratch();
    if (!buf) return hipErrorOutOfMemory;
    if (n < 1) return hipErrorInvalidValue;
    const bool vec = n % 2 == 0 && aligned16(a) && aligned16(b);
    const long long nv = vec ? n / 2 : n;
    const int grid = (int)std::max<long long>(1, std::min<long long>(MON_MAX_GRID, (nv + MON_THREADS - 1) / MON_THREADS));
    double *pv = buf;
    long long *pi = reinterpret_cast<long long *>(buf + 2 * MON_MAX_GRID);
    double *res = buf + 4 * MON_MAX_GRID;
    {
        ProfScope ps("k_extremes_partial", st, (double)n * (b ? 16.0 : 8.0));
        if (vec && b) hipLaunchKernelGGL((k_extremes_partial<2, true>), dim3(grid), dim3(MON_THREADS), 0, st, a, b, n, pv, pi);
        else if (vec) hipLaunchKernelGGL((k_extremes_partial<2, false>), dim3(grid), dim3(MON_THREADS), 0, st, a, b, n, pv, pi);
        else if (b) hipLaunchKernelGGL((k_extremes_partial<1, true>), dim3(grid), dim3(MON_THREADS), 0, st, a, b, n, pv, pi);
        else hipLaunchKernelGGL((k_extremes_partial<1, false>), dim3(grid), dim3(MON_THREADS), 0, st, a, b, n, pv, pi);
    }
    hipLaunchKernelGGL(k_extremes_final, dim3(1), dim3(MON_THREADS), 0, st, pv, pi, grid, res);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    double h[4];
    if ((e = hipMemcpyAsync(h, res, sizeof(h), hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return e;
    long long ix[2];
    std::copy(reinterpret_cast<const char *>(h + 2), reinterpret_cast<const char *>(h + 4), reinterpret_cast<char *>(ix));
    *mn = h[0]; *mx = h[1];
    if (imn) *imn = ix[0] == LLONG_MAX ? 0 : ix[0];      // (NaN everywhere: no extreme was taken; the first element, as gfortran's minloc / maxloc)
    if (imx) *imx = ix[1] == LLONG_MAX ? 0 : ix[1];
    return hipSuccess;
}

}  // namespace tlab

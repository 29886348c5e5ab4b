// Sampling between two statistics steps on the device: the phase averages of module AVG_PHASE (statistics/avg_phase.f90), the towers of module
// DNS_TOWER (tools/dns/dns_tower.f90) and the saved planes of module PLANES (tools/dns/planes.f90) with the two pointwise passes of PLANES_LOG.
//
//   k_phase_space<NF, STRESS, V>  the z-average of NF fields onto the xy-plane, localsum = localsum + field(:,:,k)/g(3)%size for k = 1..kmax
//                          (avg_phase.f90:168-174), and with STRESS of the six products of the three fields, wrk3d = f1*f2 rounded, then the same sum
//                          (:254-261).  One thread owns V consecutive points of the plane (V = 2: 16-byte accesses, the plane size even and every
//                          array 16-byte aligned; V = 1: 8-byte accesses) and keeps their NF (+ 6) sums in registers: the adds of one point go in
//                          increasing k in one thread, each term a true fp64 division by double(nz_total) -- bit for bit the reference's sum.
//                          U planes of every field are requested before the first add (U NF loads in flight per lane, 8 to 12).  No atomics, no
//                          split of k.  The fused flow form reads u, v, w ONCE for three means and six stresses (the reference: three passes plus six
//                          times write product / read product).  The same thread then stores its sums into plane plane_id of the accumulator and
//                          adds sum/avg_planes -- a division -- to the running mean in the last plane (:189-198, :276-282).
//   k_tower_gather         v(tower_ipos(ii), tower_jpos(j), tower_kpos(kk)) of up to three fields into their slots of the tower buffer, j fastest
//                          in the buffer (coalesced writes; the reads are one element per line and cannot be helped); thread 0 writes the time and
//                          the iteration of the pressure call.
//   k_tower_means          the plane means k_plane_partial / k_plane_final left in a profile, taken at the planes tower_jpos, into the buffer.
//   k_planes_gather<T>     selected i-, j- or k-planes of nvars fields as data_i(jmax, size, kmax) (transposed, planes.f90:330-338), data_j(imax,
//                          size, kmax), data_k(imax, jmax, size); T = double, or float rounded to nearest (IO_TYPE_SINGLE).  One thread per element of
//                          the output, the output's fastest index fastest: writes coalesced in every direction; the reads of an i-plane are one
//                          element per 128-byte line.
//   k_gradient_magnitude   FI_GRADIENT's two pointwise statements (fi_gradient.f90:38, :40): r = r*r + t*t, then r = r + t*t
//   k_log10_small          a = log10(a + small_wp) (planes.f90:250, :256)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <type_traits>

#include "kernels.hpp"
#include "profile.hpp"

#pragma clang fp contract(off)      // every multiply, add and division below stays as written

namespace tlab {
namespace {

constexpr int PH_THREADS = 128, SMP_THREADS = 256;

struct PhaseArgs {
    const double *f[3];
    double *out[9], *last[9];      // plane plane_id and the last plane (the running mean) of each output
    long long nxy;
    int nz;
    double dz, dplanes;            // double(nz_total), double(avg_planes)
};

// the terms of one point and one plane, in the reference's order: the means of the fields, then uu, uv, uw, vv, vw, ww
template <int NF, bool STRESS>
__device__ __forceinline__ void phase_add(const double *y, double dz, double *acc) {
#pragma unroll
    for (int f = 0; f < NF; ++f) acc[f] = acc[f] + y[f] / dz;
    if constexpr (STRESS) {
        const double uu = y[0] * y[0], uv = y[0] * y[1], uw = y[0] * y[2], vv = y[1] * y[1], vw = y[1] * y[2], ww = y[2] * y[2];
        acc[NF + 0] = acc[NF + 0] + uu / dz;
        acc[NF + 1] = acc[NF + 1] + uv / dz;
        acc[NF + 2] = acc[NF + 2] + uw / dz;
        acc[NF + 3] = acc[NF + 3] + vv / dz;
        acc[NF + 4] = acc[NF + 4] + vw / dz;
        acc[NF + 5] = acc[NF + 5] + ww / dz;
    }
}

// U planes k0 .. k0 + U - 1 of the thread's V points: every load first, then the adds in increasing k
template <int NF, bool STRESS, int V, int U>
__device__ __forceinline__ void phase_planes(const PhaseArgs &a, long long p, int k0, double (*acc)[NF + (STRESS ? 6 : 0)]) {
    using T = std::conditional_t<V == 2, double2, double>;
    T x[U][NF];
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
        for (int f = 0; f < NF; ++f) x[u][f] = *reinterpret_cast<const T *>(a.f[f] + (long long)(k0 + u) * a.nxy + p);
#pragma unroll
    for (int u = 0; u < U; ++u) {
        double y[NF];
        if constexpr (V == 2) {
#pragma unroll
            for (int f = 0; f < NF; ++f) y[f] = x[u][f].x;
            phase_add<NF, STRESS>(y, a.dz, acc[0]);
#pragma unroll
            for (int f = 0; f < NF; ++f) y[f] = x[u][f].y;
            phase_add<NF, STRESS>(y, a.dz, acc[1]);
        } else {
#pragma unroll
            for (int f = 0; f < NF; ++f) y[f] = x[u][f];
            phase_add<NF, STRESS>(y, a.dz, acc[0]);
        }
    }
}

template <int NF, bool STRESS, int V>
__global__ void __launch_bounds__(PH_THREADS) k_phase_space(const PhaseArgs a) {
    constexpr int NO = NF + (STRESS ? 6 : 0), U = NF == 1 ? 8 : 4;
    const long long p = ((long long)blockIdx.x * PH_THREADS + threadIdx.x) * V;
    if (p >= a.nxy) return;      // (V = 2: nxy is even, so p + 1 < nxy too)
    double acc[V][NO];
#pragma unroll
    for (int c = 0; c < V; ++c)
#pragma unroll
        for (int o = 0; o < NO; ++o) acc[c][o] = 0.0;
    int k = 0;
    for (; k + U <= a.nz; k += U) phase_planes<NF, STRESS, V, U>(a, p, k, acc);
    for (; k < a.nz; ++k) phase_planes<NF, STRESS, V, 1>(a, p, k, acc);
#pragma unroll
    for (int o = 0; o < NO; ++o) {
        if constexpr (V == 2) {
            double2 s, l = *reinterpret_cast<const double2 *>(a.last[o] + p);
            s.x = acc[0][o]; s.y = acc[1][o];
            l.x = l.x + s.x / a.dplanes; l.y = l.y + s.y / a.dplanes;
            *reinterpret_cast<double2 *>(a.out[o] + p) = s;
            *reinterpret_cast<double2 *>(a.last[o] + p) = l;
        } else {
            const double s = acc[0][o];
            a.out[o][p] = s;
            a.last[o][p] = a.last[o][p] + s / a.dplanes;
        }
    }
}

struct TowerArgs {
    const double *f[3];
    double *dst[3];                // the slot of this accumulation in each field's part of the buffer
    const int *ipos, *jpos, *kpos;      // 1-based
    int nf, ti, tj, tk, nx, ny;
    double *t_slot, *it_slot;      // NULL unless the pressure call
    double rtime, itime;
};

__global__ void __launch_bounds__(SMP_THREADS) k_tower_gather(const TowerArgs a) {
    const long long t = (long long)blockIdx.x * SMP_THREADS + threadIdx.x, nt = (long long)a.tj * a.ti * a.tk;
    if (t == 0 && a.t_slot) { *a.t_slot = a.rtime; *a.it_slot = a.itime; }
    if (t >= nt) return;
    const int j = (int)(t % a.tj), ii = (int)((t / a.tj) % a.ti), kk = (int)(t / ((long long)a.tj * a.ti));
    const long long src = ((long long)(a.kpos[kk] - 1) * a.ny + (a.jpos[j] - 1)) * a.nx + (a.ipos[ii] - 1);
    for (int f = 0; f < a.nf; ++f) a.dst[f][t] = a.f[f][src];
}

// dst[f][j] = prof[f][jpos[j] - 1]
__global__ void __launch_bounds__(SMP_THREADS) k_tower_means(const double *__restrict__ prof, int ny, const int *__restrict__ jpos, int tj, int nf,
                                                             double *d0, double *d1, double *d2) {
    const int t = blockIdx.x * SMP_THREADS + threadIdx.x;
    if (t >= tj * nf) return;
    const int f = t / tj, j = t % tj;
    double *dst = f == 0 ? d0 : f == 1 ? d1 : d2;
    dst[j] = prof[(size_t)f * ny + (jpos[j] - 1)];
}

struct PlanesArgs {
    const double *f[PLANES_MAX_VARS];
    int nodes[PLANES_MAX_NODES];      // 1-based
    int nvars, n, dir, nx, ny, nz;
};

template <class T>
__global__ void __launch_bounds__(SMP_THREADS) k_planes_gather(const PlanesArgs a, T *__restrict__ out, long long total) {
    const long long t = (long long)blockIdx.x * SMP_THREADS + threadIdx.x;
    if (t >= total) return;
    const int size = a.nvars * a.n;
    int slot;
    long long src;
    if (a.dir == 1) {             // data_i(j, slot, k) = field(node, j, k)
        const int j = (int)(t % a.ny), k = (int)(t / ((long long)a.ny * size));
        slot = (int)((t / a.ny) % size);
        src = ((long long)k * a.ny + j) * a.nx + (a.nodes[slot % a.n] - 1);
    } else if (a.dir == 2) {      // data_j(i, slot, k) = field(i, node, k)
        const int i = (int)(t % a.nx), k = (int)(t / ((long long)a.nx * size));
        slot = (int)((t / a.nx) % size);
        src = ((long long)k * a.ny + (a.nodes[slot % a.n] - 1)) * a.nx + i;
    } else {                      // data_k(i, j, slot) = field(i, j, node)
        const long long nxy = (long long)a.nx * a.ny;
        slot = (int)(t / nxy);
        src = (long long)(a.nodes[slot % a.n] - 1) * nxy + t % nxy;
    }
    out[t] = (T)a.f[slot / a.n][src];      // (float: round to nearest)
}

__global__ void __launch_bounds__(SMP_THREADS) k_gradient_magnitude(double *__restrict__ r, const double *__restrict__ t, int second, long long n) {
    const long long i = (long long)blockIdx.x * SMP_THREADS + threadIdx.x;
    if (i >= n) return;
    const double a = r[i], b = t[i];
    r[i] = second ? a + b * b : a * a + b * b;
}

__global__ void __launch_bounds__(SMP_THREADS) k_log10_small(double *__restrict__ a, long long n) {
    const long long i = (long long)blockIdx.x * SMP_THREADS + threadIdx.x;
    if (i < n) a[i] = log10(a[i] + 1.0e-20);
}

bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }
unsigned blocks(long long n, int threads) { return (unsigned)((n + threads - 1) / threads); }

template <int NF, bool STRESS>
void phase_launch(bool vec, const PhaseArgs &a, hipStream_t st) {
    const double bytes = 8.0 * (double)a.nxy * ((double)a.nz * NF + 3.0 * (NF + (STRESS ? 6 : 0)));
    ProfScope ps(STRESS ? "k_phase_space<flow>" : "k_phase_space", st, bytes);
    if (vec) hipLaunchKernelGGL((k_phase_space<NF, STRESS, 2>), dim3(blocks(a.nxy / 2, PH_THREADS)), dim3(PH_THREADS), 0, st, a);
    else hipLaunchKernelGGL((k_phase_space<NF, STRESS, 1>), dim3(blocks(a.nxy, PH_THREADS)), dim3(PH_THREADS), 0, st, a);
}

}  // namespace

hipError_t launch_phase_space(int nf, bool stress, const double *const *f, double *const *out, double *const *last, long long nxy, int nz, int nz_total,
                              int avg_planes, hipStream_t st) {
    const int nout = nf + (stress ? 6 : 0);
    if (nf < 1 || nf > 3 || (stress && nf != 3) || !f || !out || !last || nxy < 1 || nz < 1 || nz_total < 1 || avg_planes < 1 ||
        (nxy + PH_THREADS - 1) / PH_THREADS > 0x7fffffffLL)
        return hipErrorInvalidValue;
    PhaseArgs a{};
    bool vec = nxy % 2 == 0;
    for (int i = 0; i < nf; ++i) {
        if (!f[i]) return hipErrorInvalidValue;
        a.f[i] = f[i];
        vec = vec && aligned16(f[i]);
    }
    for (int o = 0; o < nout; ++o) {
        if (!out[o] || !last[o]) return hipErrorInvalidValue;
        a.out[o] = out[o]; a.last[o] = last[o];
        vec = vec && aligned16(out[o]) && aligned16(last[o]);
    }
    a.nxy = nxy; a.nz = nz; a.dz = (double)nz_total; a.dplanes = (double)avg_planes;
    if (stress) phase_launch<3, true>(vec, a, st);
    else if (nf == 3) phase_launch<3, false>(vec, a, st);
    else if (nf == 2) phase_launch<2, false>(vec, a, st);
    else phase_launch<1, false>(vec, a, st);
    return hipGetLastError();
}

hipError_t launch_tower_gather(int nf, const double *const *f, double *const *dst, const int *ipos, const int *jpos, const int *kpos, int ti, int tj, int tk,
                               int nx, int ny, double *t_slot, double *it_slot, double rtime, int itime, hipStream_t st) {
    if (nf < 1 || nf > 3 || !f || !dst || !ipos || !jpos || !kpos || ti < 0 || tj < 0 || tk < 0 || (t_slot == nullptr) != (it_slot == nullptr))
        return hipErrorInvalidValue;
    TowerArgs a{};
    for (int i = 0; i < nf; ++i) {
        if (!f[i] || !dst[i]) return hipErrorInvalidValue;
        a.f[i] = f[i]; a.dst[i] = dst[i];
    }
    a.ipos = ipos; a.jpos = jpos; a.kpos = kpos; a.nf = nf; a.ti = ti; a.tj = tj; a.tk = tk; a.nx = nx; a.ny = ny;
    a.t_slot = t_slot; a.it_slot = it_slot; a.rtime = rtime; a.itime = (double)itime;
    const long long nt = (long long)ti * tj * tk;
    if (nt == 0 && !t_slot) return hipSuccess;
    ProfScope ps("k_tower_gather", st, 16.0 * (double)nt * nf);
    hipLaunchKernelGGL(k_tower_gather, dim3(std::max(1u, blocks(nt, SMP_THREADS))), dim3(SMP_THREADS), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_tower_means(const double *prof, int ny, const int *jpos, int tj, int nf, double *const *dst, hipStream_t st) {
    if (!prof || !jpos || !dst || nf < 1 || nf > 3 || tj < 0) return hipErrorInvalidValue;
    if (tj == 0) return hipSuccess;
    hipLaunchKernelGGL(k_tower_means, dim3(blocks((long long)tj * nf, SMP_THREADS)), dim3(SMP_THREADS), 0, st, prof, ny, jpos, tj, nf, dst[0],
                       nf > 1 ? dst[1] : nullptr, nf > 2 ? dst[2] : nullptr);
    return hipGetLastError();
}

hipError_t launch_planes_gather(int nx, int ny, int nz, int nvars, const double *const *f, int dir, int n, const int *nodes, void *out, bool single,
                                hipStream_t st) {
    if (nx < 1 || ny < 1 || nz < 1 || nvars < 1 || nvars > PLANES_MAX_VARS || !f || dir < 1 || dir > 3 || n < 1 || n > PLANES_MAX_NODES || !nodes || !out)
        return hipErrorInvalidValue;
    const int len[3] = {nx, ny, nz};
    PlanesArgs a{};
    for (int v = 0; v < nvars; ++v) {
        if (!f[v]) return hipErrorInvalidValue;
        a.f[v] = f[v];
    }
    for (int m = 0; m < n; ++m) {
        if (nodes[m] < 1 || nodes[m] > len[dir - 1]) return hipErrorInvalidValue;      // (the kernel trusts them)
        a.nodes[m] = nodes[m];
    }
    a.nvars = nvars; a.n = n; a.dir = dir; a.nx = nx; a.ny = ny; a.nz = nz;
    const long long total = (long long)nx * ny * nz / len[dir - 1] * n * nvars;
    if ((total + SMP_THREADS - 1) / SMP_THREADS > 0x7fffffffLL) return hipErrorInvalidValue;
    ProfScope ps("k_planes_gather", st, (double)total * (8.0 + (single ? 4.0 : 8.0)));
    if (single) hipLaunchKernelGGL((k_planes_gather<float>), dim3(blocks(total, SMP_THREADS)), dim3(SMP_THREADS), 0, st, a, (float *)out, total);
    else hipLaunchKernelGGL((k_planes_gather<double>), dim3(blocks(total, SMP_THREADS)), dim3(SMP_THREADS), 0, st, a, (double *)out, total);
    return hipGetLastError();
}

hipError_t launch_gradient_magnitude(double *r, const double *t, bool second, long long n, hipStream_t st) {
    if (!r || !t || n < 1 || (n + SMP_THREADS - 1) / SMP_THREADS > 0x7fffffffLL) return hipErrorInvalidValue;
    ProfScope ps("k_gradient_magnitude", st, 24.0 * (double)n);
    hipLaunchKernelGGL(k_gradient_magnitude, dim3(blocks(n, SMP_THREADS)), dim3(SMP_THREADS), 0, st, r, t, second ? 1 : 0, n);
    return hipGetLastError();
}

hipError_t launch_log10_small(double *a, long long n, hipStream_t st) {
    if (!a || n < 1 || (n + SMP_THREADS - 1) / SMP_THREADS > 0x7fffffffLL) return hipErrorInvalidValue;
    ProfScope ps("k_log10_small", st, 16.0 * (double)n);
    hipLaunchKernelGGL(k_log10_small, dim3(blocks(n, SMP_THREADS)), dim3(SMP_THREADS), 0, st, a, n);
    return hipGetLastError();
}

}  // namespace tlab

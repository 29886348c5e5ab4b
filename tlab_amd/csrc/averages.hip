// Horizontal-plane statistics on the device: the plane averages of module Averages (utils/averages.f90: AVG_IK_V :301-327, AVG1V2D_V :142-167) and
// the moment groups of AVG_FLOW_XZ (statistics/avg_flow_xz.f90:513-553, :597-654) and AVG_SCAL_XZ (statistics/avg_scal_xz.f90:373-455) that need no
// derivative, as TWO passes over the fields (the means, then every covariance) instead of one temporary field and one reduction per output; and
// the groups of the same routines on the velocity and scalar gradients (:976-1248, :673-699; avg_scal_xz.f90:451-453, :607, :714-745) as three
// more passes over the nine gradient fields.
//
//   k_plane_partial<P, V>  grid (ny, nchunks), 256 threads: the workgroup (j, c) sums plane j over the rows k of chunk c (AVG_ROWS_PER_GROUP rows).
//                          Wave w takes the rows c R + w, + 4, ..; its lanes run along x, V = 2: 16-byte loads (nx even, every field 16-byte
//                          aligned), V = 1: 8-byte loads.  U = P::ROWS rows of every field are requested before the first is used (U NFLD
//                          loads in flight per lane, 12 to 18); the sums have no dependent chain on the loads.  The means of plane j are the
//                          same for the whole workgroup and come from the program's device table [NMEAN][ny] through scalar loads.  All NOUT
//                          sums of the program (at most 38) stay in registers; then the wave by __shfl_xor, the four waves through LDS,
//                          and thread 0 stores partial[c][j][o].
//   k_plane_final          sums the chunks of each (j, o) in chunk order and DIVIDES by real(nx nz) (avg/real(nx*nz, wp), averages.f90:320).
//
// No atomics and no workgroup that waits for or counts another: the order of summation is a function of (nx, ny, nz) and the alignment alone, so
// the same call gives the same bits on every run.  The programs -- which terms a point adds, in the reference's operation order -- are in
// averages_host.hpp, shared with the host loop.  a**4 is (a*a)*(a*a), as gfortran expands it.
// nz = 1 and lines shorter than a wave are correct but slow (one wave, few lanes): there is no second kernel for them.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "averages_host.hpp"
#include "kernels.hpp"
#include "profile.hpp"

#pragma clang fp contract(off)      // every multiply and add below stays as written

namespace tlab {
namespace {

constexpr int AVG_THREADS = 256, AVG_WAVES = AVG_THREADS / 64;

struct AvgArgs {
    const double *f[AVG_MAX_FIELDS];
    const double *means;      // [NMEAN][ny]
    double *partial;          // [nchunks][ny][NOUT]
    int nx, ny, nz;
};

// U rows (k, k + 4, ..) of one wave: row0 = offset of the first row in a field, rstride = offset from one row to the next
template <class P, int V, int U>
__device__ __forceinline__ void avg_rows(const AvgArgs &a, size_t row0, size_t rstride, int lane, const double *m, double *acc) {
    using T = std::conditional_t<V == 2, double2, double>;
    for (int i = lane * V; i < a.nx; i += 64 * V) {
        T x[U][P::NFLD];
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int f = 0; f < P::NFLD; ++f) x[u][f] = *reinterpret_cast<const T *>(a.f[f] + row0 + u * rstride + i);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            double y[P::NFLD];
            if constexpr (V == 2) {
#pragma unroll
                for (int f = 0; f < P::NFLD; ++f) y[f] = x[u][f].x;
                P::add(y, m, acc);
#pragma unroll
                for (int f = 0; f < P::NFLD; ++f) y[f] = x[u][f].y;
                P::add(y, m, acc);
            } else {
#pragma unroll
                for (int f = 0; f < P::NFLD; ++f) y[f] = x[u][f];
                P::add(y, m, acc);
            }
        }
    }
}

template <class P, int V>
__global__ void __launch_bounds__(AVG_THREADS) k_plane_partial(const AvgArgs a) {
    constexpr int U = P::ROWS;
    __shared__ double red[AVG_WAVES][P::NOUT];
    const int j = blockIdx.x, c = blockIdx.y, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int k1 = min(a.nz, (c + 1) * AVG_ROWS_PER_GROUP);
    double m[P::NMEAN > 0 ? P::NMEAN : 1];
#pragma unroll
    for (int i = 0; i < P::NMEAN; ++i) m[i] = a.means[(size_t)i * a.ny + j];
    double acc[P::NOUT];
#pragma unroll
    for (int o = 0; o < P::NOUT; ++o) acc[o] = 0.0;
    const size_t plane = (size_t)a.nx * a.ny, rstride = AVG_WAVES * plane;
    int k = c * AVG_ROWS_PER_GROUP + wave;
    for (; k + AVG_WAVES * (U - 1) < k1; k += AVG_WAVES * U) avg_rows<P, V, U>(a, (size_t)k * plane + (size_t)j * a.nx, rstride, lane, m, acc);
    for (; k < k1; k += AVG_WAVES) avg_rows<P, V, 1>(a, (size_t)k * plane + (size_t)j * a.nx, rstride, lane, m, acc);
#pragma unroll
    for (int o = 0; o < P::NOUT; ++o) {
        double s = acc[o];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
        if (lane == 0) red[wave][o] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double *out = a.partial + ((size_t)c * a.ny + j) * P::NOUT;
#pragma unroll
        for (int o = 0; o < P::NOUT; ++o) {
            double s = red[0][o];
            for (int w = 1; w < AVG_WAVES; ++w) s += red[w][o];
            out[o] = s;
        }
    }
}

// prof[o][j] = (sum over the chunks, in chunk order, of partial[c][j][o]) / denom
__global__ void __launch_bounds__(AVG_THREADS) k_plane_final(const double *__restrict__ partial, int nchunks, int ny, int nout, double denom,
                                                             double *__restrict__ prof) {
    const int t = blockIdx.x * AVG_THREADS + threadIdx.x;
    if (t >= ny * nout) return;
    const int j = t / nout, o = t % nout;
    double s = 0.0;
    for (int c = 0; c < nchunks; ++c) s += partial[((size_t)c * ny + j) * nout + o];
    prof[(size_t)o * ny + j] = s / denom;
}

bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

int plane_moments_chunks(int nz) { return (nz + AVG_ROWS_PER_GROUP - 1) / AVG_ROWS_PER_GROUP; }

hipError_t launch_plane_moments(int prog, int param, int nx, int ny, int nz, const double *const *f, const double *means, double *partial,
                                double *prof, hipStream_t st, double denom) {
    const AvgInfo info = avg_info(prog, param);
    if (nx < 1 || ny < 1 || nz < 1 || info.nfld < 1 || info.nfld > AVG_MAX_FIELDS || !f || !partial || !prof || (info.nmean > 0 && !means))
        return hipErrorInvalidValue;
    AvgArgs a{};
    bool vec = nx % 2 == 0;
    for (int i = 0; i < info.nfld; ++i) {
        if (!f[i]) return hipErrorInvalidValue;
        a.f[i] = f[i];
        vec = vec && aligned16(f[i]);
    }
    a.means = means; a.partial = partial; a.nx = nx; a.ny = ny; a.nz = nz;
    const int nchunks = plane_moments_chunks(nz);
    if (nchunks > 65535) return hipErrorInvalidValue;
    const dim3 grid((unsigned)ny, (unsigned)nchunks);
    const double bytes = 8.0 * nx * ny * (double)nz * info.nfld;
    const bool known = avg_dispatch(prog, param, [&](auto P) {
        using Prog = decltype(P);
        ProfScope ps(Prog::TAG, st, bytes);
        if (vec) hipLaunchKernelGGL((k_plane_partial<Prog, 2>), grid, dim3(AVG_THREADS), 0, st, a);
        else hipLaunchKernelGGL((k_plane_partial<Prog, 1>), grid, dim3(AVG_THREADS), 0, st, a);
    });
    if (!known) return hipErrorInvalidValue;
    const long long nt = (long long)ny * info.nout;
    hipLaunchKernelGGL(k_plane_final, dim3((unsigned)((nt + AVG_THREADS - 1) / AVG_THREADS)), dim3(AVG_THREADS), 0, st, partial, nchunks, ny, info.nout,
                       denom != 0.0 ? denom : (double)((long long)nx * nz), prof);
    return hipGetLastError();
}

}  // namespace tlab

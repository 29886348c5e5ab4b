// Field mappings of the reference's mappings/ directory as ONE streaming pass over the velocity and scalar gradients (k_gradient_maps), and the two
// accumulate kernels of the terms composed from second derivatives (mappings.cpp).  Every first-derivative mapping -- FI_INVARIANT_P/Q/R,
// FI_STRAIN, FI_STRAIN_TENSOR, FI_CURL, FI_VORTICITY, FI_VORTICITY_PRODUCTION, FI_STRAIN_PRODUCTION, FI_GRADIENT, FI_GRADIENT_PRODUCTION, FI_STRAIN_A
// -- is a pointwise function of u,x .. w,z and s,x s,y s,z: where the reference takes its derivatives again for every routine and makes a
// two-operand pass per statement, the pass reads each gradient once and writes each output once.  The arithmetic of a point is
// gradient_maps_point (mappings_host.hpp), shared with the host loop: unfused, in the reference's operation order.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "mappings_host.hpp"
#include "profile.hpp"

namespace tlab {

// V = 2: 16-byte accesses (every array of the call 16-byte aligned), the odd last point by one thread; V = 1: 8-byte accesses.  The selection
// (A.maps, A.needs) is uniform over the launch: the branches are scalar, an input no requested map needs is not loaded, an output not asked for
// is not stored.  No LDS, no atomics; the arrays g, o are indexed by constants only and live in registers.
template <int V>
__device__ __forceinline__ void gradient_maps_at(const GradientMapArgs &A, long long i) {
    double g[V][MAP_INPUTS], o[V][MAP_OUTPUTS];
#pragma unroll
    for (int k = 0; k < MAP_INPUTS; ++k) {
        if (A.needs >> k & 1u) {
            if constexpr (V == 2) {
                const double2 t = reinterpret_cast<const double2 *>(A.in[k])[i];
                g[0][k] = t.x; g[1][k] = t.y;
            } else {
                g[0][k] = A.in[k][i];
            }
        } else {
#pragma unroll
            for (int v = 0; v < V; ++v) g[v][k] = 0.0;
        }
    }
#pragma unroll
    for (int v = 0; v < V; ++v) gradient_maps_point(A.maps, g[v], o[v]);
#pragma unroll
    for (int m = 0; m < MAP_COUNT; ++m) {
        if (A.maps >> m & 1u) {
#pragma unroll
            for (int k = MAP_FIRST[m]; k < MAP_FIRST[m] + MAP_NOUT[m]; ++k) {
                if constexpr (V == 2) reinterpret_cast<double2 *>(A.out[k])[i] = make_double2(o[0][k], o[1][k]);
                else A.out[k][i] = o[0][k];
            }
        }
    }
}
template <int V>
__global__ void __launch_bounds__(GRADIENT_MAPS_THREADS) k_gradient_maps(GradientMapArgs A, long long n) {
    const long long stride = (long long)gridDim.x * blockDim.x, i0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if constexpr (V == 2) {
        const long long n2 = n >> 1;
        for (long long i = i0; i < n2; i += stride) gradient_maps_at<2>(A, i);
        if ((n & 1) && i0 == 0) gradient_maps_at<1>(A, n - 1);
    } else {
        for (long long i = i0; i < n; i += stride) gradient_maps_at<1>(A, i);
    }
}

static int maps_grid(long long items) {
    const long long b = (items + GRADIENT_MAPS_THREADS - 1) / GRADIENT_MAPS_THREADS;
    return (int)(b < GRADIENT_MAPS_MAX_BLOCKS ? (b < 1 ? 1 : b) : GRADIENT_MAPS_MAX_BLOCKS);
}

hipError_t launch_gradient_maps(const GradientMapArgs &A, long long n, hipStream_t st) {
    if (n < 1 || n > 0x7fffffffLL || A.maps == 0u || A.maps >> MAP_COUNT) return hipErrorInvalidValue;
    uintptr_t bits = 0;
    double streams = 0.0;
    for (int k = 0; k < MAP_INPUTS; ++k)
        if (A.needs >> k & 1u) {
            if (!A.in[k]) return hipErrorInvalidValue;
            bits |= (uintptr_t)A.in[k];
            streams += 1.0;
        }
    for (int m = 0; m < MAP_COUNT; ++m)
        if (A.maps >> m & 1u)
            for (int k = MAP_FIRST[m]; k < MAP_FIRST[m] + MAP_NOUT[m]; ++k) {
                if (!A.out[k]) return hipErrorInvalidValue;
                bits |= (uintptr_t)A.out[k];
                streams += 1.0;
            }
    ProfScope ps("k_gradient_maps", st, (double)n * 8.0 * streams);
    if ((bits & 15) == 0) hipLaunchKernelGGL(k_gradient_maps<2>, dim3(maps_grid((n + 1) / 2)), dim3(GRADIENT_MAPS_THREADS), 0, st, A, n);
    else hipLaunchKernelGGL(k_gradient_maps<1>, dim3(maps_grid(n)), dim3(GRADIENT_MAPS_THREADS), 0, st, A, n);
    return hipGetLastError();
}

// r = [r +] (c f) ((t1 + t2) + t3): a term `strain*(tmp1 + tmp2 + tmp3)` of FI_VORTICITY_DIFFUSION, FI_STRAIN_DIFFUSION (c = 0.5 for the
// off-diagonal components: 0.5_wp*strain*(..) is (0.5*strain)*(..); c = 1 multiplies exactly) and FI_GRADIENT_DIFFUSION
template <bool ACC>
__global__ void __launch_bounds__(256) k_acc_prod3(double *__restrict__ r, double c, const double *__restrict__ f, const double *__restrict__ t1,
                                                   const double *__restrict__ t2, const double *__restrict__ t3, long long n) {
#pragma clang fp contract(off)
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const double t = (c * f[i]) * ((t1[i] + t2[i]) + t3[i]);
        r[i] = ACC ? r[i] + t : t;
    }
}
// r = [r +] a (b [+ c]): a term `tmp1*tmp2` or `tmp1*(tmp2 + tmp3)` of FI_STRAIN_PRESSURE
template <bool ACC, bool SUM>
__global__ void __launch_bounds__(256) k_acc_prod2(double *__restrict__ r, const double *__restrict__ a, const double *__restrict__ b,
                                                   const double *__restrict__ c, long long n) {
#pragma clang fp contract(off)
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const double t = SUM ? a[i] * (b[i] + c[i]) : a[i] * b[i];
        r[i] = ACC ? r[i] + t : t;
    }
}

hipError_t launch_acc_prod3(double *r, double c, const double *f, const double *t1, const double *t2, const double *t3, int acc, long long n,
                            hipStream_t st) {
    if (!r || !f || !t1 || !t2 || !t3 || n < 1) return hipErrorInvalidValue;
    ProfScope ps("k_acc_prod3", st, (double)n * (acc ? 48.0 : 40.0));
    if (acc) hipLaunchKernelGGL(k_acc_prod3<true>, dim3(maps_grid(n)), dim3(256), 0, st, r, c, f, t1, t2, t3, n);
    else hipLaunchKernelGGL(k_acc_prod3<false>, dim3(maps_grid(n)), dim3(256), 0, st, r, c, f, t1, t2, t3, n);
    return hipGetLastError();
}
hipError_t launch_acc_prod2(double *r, const double *a, const double *b, const double *c, int acc, long long n, hipStream_t st) {
    if (!r || !a || !b || n < 1) return hipErrorInvalidValue;
    ProfScope ps("k_acc_prod2", st, (double)n * ((acc ? 32.0 : 24.0) + (c ? 8.0 : 0.0)));
    const dim3 grid(maps_grid(n)), block(256);
    if (acc && c) hipLaunchKernelGGL((k_acc_prod2<true, true>), grid, block, 0, st, r, a, b, c, n);
    else if (acc) hipLaunchKernelGGL((k_acc_prod2<true, false>), grid, block, 0, st, r, a, b, c, n);
    else if (c) hipLaunchKernelGGL((k_acc_prod2<false, true>), grid, block, 0, st, r, a, b, c, n);
    else hipLaunchKernelGGL((k_acc_prod2<false, false>), grid, block, 0, st, r, a, b, c, n);
    return hipGetLastError();
}

}  // namespace tlab

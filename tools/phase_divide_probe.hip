// Is k_phase_space bound by its divisions or by its bytes?  The fused flow form of csrc/sampling.hip (three fields read once, three means and six
// products summed over k in one thread, every term DIVIDED by nz_total: 9 fp64 divisions per point and plane) next to the same loop with the
// division replaced by a multiplication by the reciprocal -- which is NOT the reference's arithmetic and therefore lives here, in a measuring
// tool, and never in the library.  Same loads, same unroll, same block size; HIP events around each launch, medians of `reps` launches after a
// warm-up, alternated.  tools/sampling_time.py runs it as a child process.
//   phase_divide_probe [n = 512] [reps = 15]     prints one JSON line
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#pragma clang fp contract(off)

#define CK(e)                                                                     \
    do {                                                                          \
        hipError_t e_ = (e);                                                      \
        if (e_ != hipSuccess) {                                                   \
            std::fprintf(stderr, "%s: %s\n", #e, hipGetErrorString(e_));          \
            return 1;                                                             \
        }                                                                         \
    } while (0)

constexpr int THREADS = 128, U = 4;

template <bool DIVIDE>
__device__ __forceinline__ double term(double x, double dz, double rdz) {
    if constexpr (DIVIDE) return x / dz;
    else return x * rdz;
}

template <bool DIVIDE>
__global__ void __launch_bounds__(THREADS) k_probe(const double *__restrict__ u, const double *__restrict__ v, const double *__restrict__ w,
                                                   double *__restrict__ out, long long nxy, int nz, double dz) {
    const long long p = ((long long)blockIdx.x * THREADS + threadIdx.x) * 2;
    if (p >= nxy) return;
    const double rdz = 1.0 / dz;
    double acc[2][9];
    for (int c = 0; c < 2; ++c)
        for (int o = 0; o < 9; ++o) acc[c][o] = 0.0;
    for (int k = 0; k + U <= nz; k += U) {      // (nz is a multiple of U here)
        double2 x[U][3];
#pragma unroll
        for (int i = 0; i < U; ++i) {
            x[i][0] = *reinterpret_cast<const double2 *>(u + (long long)(k + i) * nxy + p);
            x[i][1] = *reinterpret_cast<const double2 *>(v + (long long)(k + i) * nxy + p);
            x[i][2] = *reinterpret_cast<const double2 *>(w + (long long)(k + i) * nxy + p);
        }
#pragma unroll
        for (int i = 0; i < U; ++i)
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const double a = c ? x[i][0].y : x[i][0].x, b = c ? x[i][1].y : x[i][1].x, d = c ? x[i][2].y : x[i][2].x;
                const double y[9] = {a, b, d, a * a, a * b, a * d, b * b, b * d, d * d};
#pragma unroll
                for (int o = 0; o < 9; ++o) acc[c][o] = acc[c][o] + term<DIVIDE>(y[o], dz, rdz);
            }
    }
    for (int o = 0; o < 9; ++o) {
        double2 s;
        s.x = acc[0][o]; s.y = acc[1][o];
        *reinterpret_cast<double2 *>(out + (long long)o * nxy + p) = s;
    }
}

__global__ void k_fill(double *a, long long n, double scale) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) a[i] = scale * (double)((i * 2654435761LL) % 1000003) / 1000003.0 - 0.5;
}

int main(int argc, char **argv) {
    const int n = argc > 1 ? std::atoi(argv[1]) : 512, reps = argc > 2 ? std::atoi(argv[2]) : 15;
    if (n < 4 || n % 4 != 0 || n > 1024 || reps < 1) { std::fprintf(stderr, "n: a multiple of 4 up to 1024; reps >= 1\n"); return 2; }
    const long long nxy = (long long)n * n, total = nxy * n;
    double *f[3], *out;
    for (double *&p : f) {
        CK(hipMalloc((void **)&p, total * sizeof(double)));
        hipLaunchKernelGGL(k_fill, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, 0, p, total, 1.0 + (&p - f));
    }
    CK(hipMalloc((void **)&out, 9 * nxy * sizeof(double)));
    CK(hipDeviceSynchronize());
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    const dim3 grid((unsigned)((nxy / 2 + THREADS - 1) / THREADS));
    std::vector<float> ms[2];
    for (int r = -3; r < reps; ++r)      // three warm-up rounds; the two forms alternate
        for (int form = 0; form < 2; ++form) {
            CK(hipEventRecord(e0, 0));
            if (form == 0) hipLaunchKernelGGL((k_probe<true>), grid, dim3(THREADS), 0, 0, f[0], f[1], f[2], out, nxy, n, (double)n);
            else hipLaunchKernelGGL((k_probe<false>), grid, dim3(THREADS), 0, 0, f[0], f[1], f[2], out, nxy, n, (double)n);
            CK(hipEventRecord(e1, 0));
            CK(hipEventSynchronize(e1));
            float t;
            CK(hipEventElapsedTime(&t, e0, e1));
            if (r >= 0) ms[form].push_back(t);
        }
    CK(hipGetLastError());
    for (auto &v : ms) std::sort(v.begin(), v.end());
    const double bytes = 8.0 * (3.0 * (double)total + 9.0 * (double)nxy), md = ms[0][reps / 2], mm = ms[1][reps / 2];
    std::printf("{\"n\": %d, \"reps\": %d, \"bytes\": %.0f, \"divide_ms_median\": %.4f, \"divide_ms_min\": %.4f, \"divide_ms_max\": %.4f, "
                "\"multiply_ms_median\": %.4f, \"multiply_ms_min\": %.4f, \"multiply_ms_max\": %.4f, \"divide_TBps\": %.3f, \"multiply_TBps\": %.3f}\n",
                n, reps, bytes, md, ms[0].front(), ms[0].back(), mm, ms[1].front(), ms[1].back(), bytes / (md * 1e-3) / 1e12, bytes / (mm * 1e-3) / 1e12);
    for (double *p : f) CK(hipFree(p));
    CK(hipFree(out));
    return 0;
}

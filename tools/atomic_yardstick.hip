// The fp64 atomic-add rate of one MI355X in its best shape, as a yardstick for k_particle_deposit (tools/particle_transfers_time.py runs it as a
// child process): consecutive lanes add to consecutive doubles of a 1-GiB array, one no-return agent-scope add per lane, every double of the array
// once per launch.
//   hipcc -O3 --offload-arch=gfx950 tools/atomic_yardstick.hip -o tools/atomic_yardstick && tools/atomic_yardstick [doubles]
// Prints one JSON line: added bytes / median launch time (HIP events, 10 launches after 2 warm-ups).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CK(x)                                                                              \
    do {                                                                                   \
        hipError_t e_ = (x);                                                               \
        if (e_ != hipSuccess) {                                                            \
            fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e_));      \
            exit(1);                                                                       \
        }                                                                                  \
    } while (0)

__global__ void __launch_bounds__(256) add8(double *a, long long n) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) (void)__hip_atomic_fetch_add(a + i, 1.0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

int main(int argc, char **argv) {
    const long long n = argc > 1 ? atoll(argv[1]) : (1LL << 27);      // 1 GiB of doubles
    if (n < 1 || n > (1LL << 31)) { fprintf(stderr, "doubles: 1 .. 2^31\n"); return 1; }
    double *a = nullptr;
    CK(hipMalloc((void **)&a, (size_t)n * sizeof(double)));
    CK(hipMemset(a, 0, (size_t)n * sizeof(double)));
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    const unsigned nb = (unsigned)((n + 255) / 256);
    std::vector<float> ms;
    for (int it = 0; it < 12; ++it) {
        CK(hipEventRecord(e0, 0));
        hipLaunchKernelGGL(add8, dim3(nb), dim3(256), 0, 0, a, n);
        CK(hipGetLastError());
        CK(hipEventRecord(e1, 0));
        CK(hipEventSynchronize(e1));
        float t = 0.f;
        CK(hipEventElapsedTime(&t, e0, e1));
        if (it >= 2) ms.push_back(t);
    }
    double first = 0.0, last = 0.0;
    CK(hipMemcpy(&first, a, sizeof(double), hipMemcpyDeviceToHost));
    CK(hipMemcpy(&last, a + (n - 1), sizeof(double), hipMemcpyDeviceToHost));
    std::sort(ms.begin(), ms.end());
    const double med = 0.5 * (ms[4] + ms[5]);
    printf("{\"kernel\": \"atomic_add_f64_contiguous\", \"doubles\": %lld, \"ms\": %.4f, \"TBps_added\": %.4f, \"sums_ok\": %s}\n", n, med,
           8.0 * (double)n / (med * 1e-3) / 1e12, first == 12.0 && last == 12.0 ? "true" : "false");
    CK(hipFree(a));
    return 0;
}

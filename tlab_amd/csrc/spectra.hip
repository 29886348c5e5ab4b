// Spectra and correlations in horizontal planes on the device: what tools/statistics/spectra.f90 does between and behind the transforms of
// OPR_Fourier_CONVOLUTION_FXZ (operators/opr_fourier.f90:528-582) -- the product, the two scalings, REDUCE_SPECTRUM, INTEGRATE_SPECTRUM and
// REDUCE_CORRELATION of module SpectraMod (tools/statistics/spectra_pool.f90).  Index maps and ring lists: spectra_host.hpp.
//
//   k_spectrum_reduce<V>   ONE read of a^ (and b^): a wave per line (kz, block of nblock planes), lanes along kx.  Per mode P = Re(b^ conj(a^)),
//                          (P*norm)*norm; the block's sum goes to S(nx/2, ny/nblock, nz) at the SHUFFLED position of kz (the reference's
//                          fft_reordering_k as an index), and the Parseval sum of every line (kx = 0 once, the others twice, the Nyquist column
//                          once; :256-268) through a butterfly of __shfl_xor to rowv(nz, ny).  V = 2: 16-byte loads of a complex number.
//   k_spectrum_x           outx(kx, jb) += sum over the positions ks, ascending, of S -- the reference's own order (:82, :126) -- and, when asked
//                          for, out2d += S on the way
//   k_spectrum_z           a wave per (folded kz, jb): the (at most four) lines of S that INTEGRATE_SPECTRUM folds onto it (:84-88, :153-163), ascending, each
//                          summed along kx with the kx = 0 column left out for the first half and the mean mode's columns added twice (:103-114)
//   k_spectrum_r           a wave per (ring, jb): the modes of the ring from the list, 64 at a time
//   k_spectrum_variance    variance(j) = sum over ks, ascending, of rowv; 0 for the planes that nblock drops
//   k_cross_product        c = b^ conj(a^) (|a^|^2 for an auto pair), in place
//   k_correlation_reduce   REDUCE_CORRELATION's 2-D part: a thread per (i, jb, k) sums ((in*norm)*norm)*normj over the block's planes, ascending,
//                          into data_2d, row k = 0 into data_x, column i = 0 into data_z, and writes variance2 -- or, without data_2d, the
//                          threads of that row and column alone
//   k_correlation_r        a wave per (ring, jb), as k_spectrum_r, on the field itself
//   k_fluctuation          out = in - mean(j)
//
// No atomics, no workgroup that waits for another.  Every sum is either one thread's running sum in a stated order or a wave's: lane l takes the
// elements l, l + 64, .. in order and the 64 lane sums meet in the __shfl_xor butterfly 32, 16, .., 1, which gives every lane the same bits.  Which
// elements a lane takes depends on (nx, nz, kr_total) alone, never on the grid: the same call gives the same bits on every run.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.hpp"
#include "profile.hpp"
#include "spectra_host.hpp"

#pragma clang fp contract(off)      // every multiply and add below stays as written

namespace tlab {
namespace {

constexpr int SPEC_THREADS = 256, SPEC_WAVES = SPEC_THREADS / 64;

__device__ __forceinline__ double wave_sum(double s) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
    return s;
}

struct SpecArgs {
    const double *a, *b;      // complex (nxh, ny, nz), natural kz; b == nullptr: an auto pair
    double *S, *rowv;         // S(nkx, nyo, nz) shuffled kz; rowv(nz, ny) shuffled kz
    int nx, ny, nz, nblock, nyo;
    double norm;
};

template <int V>
__device__ __forceinline__ double2 load_c(const double *p, size_t i) {
    if constexpr (V == 2) return *reinterpret_cast<const double2 *>(p + 2 * i);
    else return make_double2(p[2 * i], p[2 * i + 1]);
}

template <int V>
__global__ void __launch_bounds__(SPEC_THREADS) k_spectrum_reduce(const SpecArgs g) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long long line = (long long)blockIdx.x * SPEC_WAVES + wave;
    if (line >= (long long)g.nyo * g.nz) return;      // (no barrier below)
    const int kn = (int)(line / g.nyo), jb = (int)(line % g.nyo), ks = spec_shifted(kn, g.nz);
    const int nkx = g.nx / 2, nxh = nkx + 1;
    double *Srow = g.S + ((size_t)ks * g.nyo + jb) * nkx;
    for (int jj = 0; jj < g.nblock; ++jj) {
        const int j = jb * g.nblock + jj;
        const size_t base = ((size_t)kn * g.ny + j) * nxh;
        double v = 0.0;
        for (int i = lane; i < nxh; i += 64) {
            const double2 a = load_c<V>(g.a, base + i);
            const double2 b = g.b ? load_c<V>(g.b, base + i) : a;
            double p = b.x * a.x + b.y * a.y;
            p = (p * g.norm) * g.norm;
            if (i < nkx) {
                Srow[i] = jj == 0 ? p : Srow[i] + p;      // (this lane's element alone)
                v += i == 0 ? p : p * 2.0;
            } else v += p;
        }
        v = wave_sum(v);
        if (lane == 0) g.rowv[(size_t)j * g.nz + ks] = v;
    }
}

__global__ void __launch_bounds__(SPEC_THREADS) k_spectrum_x(const double *__restrict__ S, int nkx, int nyo, int nz, double *__restrict__ outx,
                                                             double *__restrict__ out2d) {
    const long long t = (long long)blockIdx.x * SPEC_THREADS + threadIdx.x;
    if (t >= (long long)nkx * nyo) return;
    const size_t plane = (size_t)nkx * nyo;
    double s = 0.0;
    for (int ks = 0; ks < nz; ++ks) {
        const double p = S[ks * plane + t];
        s += p;
        if (out2d) out2d[ks * plane + t] += p;
    }
    outx[t] += s;
}

__global__ void __launch_bounds__(SPEC_THREADS) k_spectrum_z(const double *__restrict__ S, int nkx, int nyo, int nz, double *__restrict__ outz) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nkz = nz / 2;
    const long long w = (long long)blockIdx.x * SPEC_WAVES + wave;
    if (w >= (long long)nkz * nyo) return;
    const int jb = (int)(w / nkz), kzf = (int)(w % nkz);
    // the positions (1-based, ascending) that fold onto kz_global = kzf + 1: the first position when that is the Nyquist mode's neighbour,
    // nz/2 - kz_global + 2 of the first half, kz_global + nz/2 of the second, and with odd nz the last one; each is held to spec_fold itself
    const int h = nz / 2, cand[4] = {1, h - kzf + 1, kzf + 1 + h, 2 * h + 1};
    double total = 0.0;
    int last = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int ks = cand[c] - 1;
        if (cand[c] <= last || cand[c] < 1 || cand[c] > nz) continue;
        const SpecFold f = spec_fold(ks, nz);
        if (f.kzg1 - 1 != kzf) continue;
        last = cand[c];
        const double *row = S + ((size_t)ks * nyo + jb) * nkx;
        double t = 0.0;
        for (int i = lane; i < nkx; i += 64) {
            const double p = row[i];
            if (i == 0) { if (f.flag == 0) t += p; }
            else {
                t += p;
                if (f.kzg1 == 1) t += p;
            }
        }
        total += wave_sum(t);
    }
    if (lane == 0) outz[(size_t)jb * nkz + kzf] += total;
}

// S(nkx, nyo, nz): mode m = kx + nkx * ks of plane block jb at (ks * nyo + jb) * nkx + kx
__global__ void __launch_bounds__(SPEC_THREADS) k_spectrum_r(const double *__restrict__ S, int nkx, int nyo, int kr_total, const int *__restrict__ off,
                                                             const int *__restrict__ mode, double *__restrict__ outr) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long long w = (long long)blockIdx.x * SPEC_WAVES + wave;
    if (w >= (long long)kr_total * nyo) return;
    const int jb = (int)(w / kr_total), r = (int)(w % kr_total);
    double t = 0.0;
    for (int m = off[r] + lane; m < off[r + 1]; m += 64) {
        const int ks = mode[m] / nkx, i = mode[m] % nkx;
        t += S[((size_t)ks * nyo + jb) * nkx + i];
    }
    t = wave_sum(t);
    if (lane == 0) outr[(size_t)jb * kr_total + r] += t;
}

__global__ void __launch_bounds__(SPEC_THREADS) k_spectrum_variance(const double *__restrict__ rowv, int ny, int ny_loc, int nz, double *__restrict__ variance) {
    const int j = blockIdx.x * SPEC_THREADS + threadIdx.x;
    if (j >= ny) return;
    double s = 0.0;
    if (j < ny_loc)
        for (int ks = 0; ks < nz; ++ks) s += rowv[(size_t)j * nz + ks];
    variance[j] = s;
}

__global__ void __launch_bounds__(SPEC_THREADS) k_cross_product(const double *a, const double *b, double *c, long long n) {
    const long long i = (long long)blockIdx.x * SPEC_THREADS + threadIdx.x;
    if (i >= n) return;
    const double ar = a[2 * i], ai = a[2 * i + 1];
    const double br = b ? b[2 * i] : ar, bi = b ? b[2 * i + 1] : ai;
    c[2 * i] = br * ar + bi * ai;
    c[2 * i + 1] = bi * ar - br * ai;
}

struct CorrArgs {
    const double *in, *normj;      // in(nx, ny, nz); normj(ny): 1/(sqrt(var1) sqrt(var2)) or 1
    double *out2d, *outx, *outz, *variance2;
    int nx, ny, nz, nblock, nyo;
    double norm;
};

// the block's sum of one separation (i, k), and variance2 from the thread of (0, 0)
__device__ __forceinline__ double corr_point(const CorrArgs &g, int i, int jb, int k) {
    double s = 0.0;
    for (int jj = 0; jj < g.nblock; ++jj) {
        const int j = jb * g.nblock + jj;
        const double x = (g.in[((size_t)k * g.ny + j) * g.nx + i] * g.norm) * g.norm;
        if (i == 0 && k == 0 && g.variance2) g.variance2[j] = x;
        s += x * g.normj[j];
    }
    return s;
}

__global__ void __launch_bounds__(SPEC_THREADS) k_correlation_reduce(const CorrArgs g) {
    const long long t = (long long)blockIdx.x * SPEC_THREADS + threadIdx.x;
    if (g.out2d) {
        if (t >= (long long)g.nx * g.nyo * g.nz) return;
        const int i = (int)(t % g.nx), jb = (int)((t / g.nx) % g.nyo), k = (int)(t / ((long long)g.nx * g.nyo));
        const double s = corr_point(g, i, jb, k);
        g.out2d[t] += s;
        if (k == 0) g.outx[(size_t)jb * g.nx + i] += s;
        if (i == 0) g.outz[(size_t)jb * g.nz + k] += s;
    } else {      // row k = 0, then column i = 0, of every block
        const int n = g.nx + g.nz;
        if (t >= (long long)n * g.nyo) return;
        const int jb = (int)(t / n), e = (int)(t % n);
        if (e < g.nx) g.outx[(size_t)jb * g.nx + e] += corr_point(g, e, jb, 0);
        else {
            CorrArgs h = g;
            h.variance2 = nullptr;      // (written by the thread of the row)
            g.outz[(size_t)jb * g.nz + (e - g.nx)] += corr_point(h, 0, jb, e - g.nx);
        }
    }
}

__global__ void __launch_bounds__(SPEC_THREADS) k_correlation_r(const CorrArgs g, int nr_total, const int *__restrict__ off, const int *__restrict__ mode,
                                                                double *__restrict__ outr) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long long w = (long long)blockIdx.x * SPEC_WAVES + wave;
    if (w >= (long long)nr_total * g.nyo) return;
    const int jb = (int)(w / nr_total), r = (int)(w % nr_total);
    CorrArgs h = g;
    h.variance2 = nullptr;
    double t = 0.0;
    for (int m = off[r] + lane; m < off[r + 1]; m += 64) t += corr_point(h, mode[m] % g.nx, jb, mode[m] / g.nx);
    t = wave_sum(t);
    if (lane == 0) outr[(size_t)jb * nr_total + r] += t;
}

__global__ void __launch_bounds__(SPEC_THREADS) k_fluctuation(const double *__restrict__ in, const double *__restrict__ mean, int nx, int ny,
                                                              long long n, double *__restrict__ out) {
    const long long t = (long long)blockIdx.x * SPEC_THREADS + threadIdx.x;
    if (t >= n) return;
    out[t] = in[t] - mean[(t / nx) % ny];
}

unsigned blocks(long long n, int per) { return (unsigned)((n + per - 1) / per); }
bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

hipError_t launch_spectrum_reduce(int nx, int ny, int nz, int nblock, int kr_total, const double *a, const double *b, double *S, double *rowv,
                                  const int *ring_off, const int *ring_mode, double *out2d, double *outx, double *outz, double *outr,
                                  double *variance, hipStream_t st) {
    if (nx < 2 || nx % 2 || ny < 1 || nz < 2 || nblock < 1 || nblock > ny || kr_total < 1 || !a || !S || !rowv || !ring_off || !ring_mode || !outx ||
        !outz || !outr || !variance)
        return hipErrorInvalidValue;
    const int nyo = ny / nblock, nkx = nx / 2;
    const long long lines = (long long)nyo * nz;
    if (lines > 0x7fffffffLL * SPEC_WAVES || (long long)nkx * nz > 0x7fffffffLL) return hipErrorInvalidValue;
    const SpecArgs g{a, b, S, rowv, nx, ny, nz, nblock, nyo, 1.0 / (double)((long long)nx * nz)};
    {
        ProfScope ps("k_spectrum_reduce", st, 16.0 * (nkx + 1) * (double)nyo * nblock * nz * (b ? 2 : 1) + 8.0 * nkx * (double)nyo * nz);
        if (aligned16(a) && (!b || aligned16(b))) hipLaunchKernelGGL(k_spectrum_reduce<2>, dim3(blocks(lines, SPEC_WAVES)), dim3(SPEC_THREADS), 0, st, g);
        else hipLaunchKernelGGL(k_spectrum_reduce<1>, dim3(blocks(lines, SPEC_WAVES)), dim3(SPEC_THREADS), 0, st, g);
    }
    {
        ProfScope ps("k_spectrum_x", st, 8.0 * nkx * (double)nyo * nz * (out2d ? 3 : 1));
        hipLaunchKernelGGL(k_spectrum_x, dim3(blocks((long long)nkx * nyo, SPEC_THREADS)), dim3(SPEC_THREADS), 0, st, S, nkx, nyo, nz, outx, out2d);
    }
    {
        ProfScope ps("k_spectrum_z", st, 8.0 * nkx * (double)nyo * nz);
        hipLaunchKernelGGL(k_spectrum_z, dim3(blocks((long long)(nz / 2) * nyo, SPEC_WAVES)), dim3(SPEC_THREADS), 0, st, S, nkx, nyo, nz, outz);
    }
    {
        ProfScope ps("k_spectrum_r", st, 8.0 * nkx * (double)nyo * nz);
        hipLaunchKernelGGL(k_spectrum_r, dim3(blocks((long long)kr_total * nyo, SPEC_WAVES)), dim3(SPEC_THREADS), 0, st, S, nkx, nyo, kr_total, ring_off,
                           ring_mode, outr);
    }
    hipLaunchKernelGGL(k_spectrum_variance, dim3(blocks(ny, SPEC_THREADS)), dim3(SPEC_THREADS), 0, st, rowv, ny, nyo * nblock, nz, variance);
    return hipGetLastError();
}

hipError_t launch_cross_product(const double *a, const double *b, double *c, long long n, hipStream_t st) {
    if (!a || !c || n < 1) return hipErrorInvalidValue;
    ProfScope ps("k_cross_product", st, 16.0 * (double)n * (b ? 3 : 2));
    hipLaunchKernelGGL(k_cross_product, dim3(blocks(n, SPEC_THREADS)), dim3(SPEC_THREADS), 0, st, a, b, c, n);
    return hipGetLastError();
}

hipError_t launch_correlation_reduce(int nx, int ny, int nz, int nblock, int nr_total, const double *in, const double *normj, const int *ring_off,
                                     const int *ring_mode, double *out2d, double *outx, double *outz, double *outr, double *variance2,
                                     hipStream_t st) {
    if (nx < 1 || ny < 1 || nz < 1 || nblock < 1 || nblock > ny || !in || !normj || !outx || !outz || !variance2) return hipErrorInvalidValue;
    if (outr && (nr_total < 1 || !ring_off || !ring_mode)) return hipErrorInvalidValue;
    if ((long long)nx * nz > 0x7fffffffLL) return hipErrorInvalidValue;
    const int nyo = ny / nblock;
    const CorrArgs g{in, normj, out2d, outx, outz, variance2, nx, ny, nz, nblock, nyo, 1.0 / (double)((long long)nx * nz)};
    hipError_t e = hipMemsetAsync(variance2, 0, (size_t)ny * sizeof(double), st);      // the planes that nblock drops
    if (e != hipSuccess) return e;
    {
        const long long n = out2d ? (long long)nx * nyo * nz : (long long)(nx + nz) * nyo;
        ProfScope ps("k_correlation_reduce", st, out2d ? 8.0 * nx * (double)nyo * nz * (nblock + 2) : 8.0 * (nx + nz) * (double)nyo * (nblock + 2));
        hipLaunchKernelGGL(k_correlation_reduce, dim3(blocks(n, SPEC_THREADS)), dim3(SPEC_THREADS), 0, st, g);
    }
    if (outr) {
        // the separations with i*i + k*k < nr_total**2: about a quarter disc, read in every plane of a block
        const double nsep = 0.7854 * (double)std::min(nr_total, nx) * (double)std::min(nr_total, nz);
        ProfScope ps("k_correlation_r", st, 8.0 * nsep * (double)nyo * nblock);
        hipLaunchKernelGGL(k_correlation_r, dim3(blocks((long long)nr_total * nyo, SPEC_WAVES)), dim3(SPEC_THREADS), 0, st, g, nr_total, ring_off, ring_mode,
                           outr);
    }
    return hipGetLastError();
}

hipError_t launch_fluctuation(int nx, int ny, int nz, const double *in, const double *mean, double *out, hipStream_t st) {
    if (nx < 1 || ny < 1 || nz < 1 || !in || !mean || !out) return hipErrorInvalidValue;
    const long long n = (long long)nx * ny * nz;
    ProfScope ps("k_fluctuation", st, 16.0 * (double)n);
    hipLaunchKernelGGL(k_fluctuation, dim3(blocks(n, SPEC_THREADS)), dim3(SPEC_THREADS), 0, st, in, mean, nx, ny, n, out);
    return hipGetLastError();
}

}  // namespace tlab

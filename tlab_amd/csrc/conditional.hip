// Conditional statistics on the device: the partition of FI_GATE (mappings/fi_gate.f90:65-90), the gated moments of AVG_N_XZ over AVG1V2D /
// AVG1V2D1G (statistics/avg_xz.f90:10-70, utils/averages.f90:114-137, :172-209) for every plane, level and moment in one pass, and the conditional
// averages of CAVG1V_N / CAVG2V (statistics/cavg.f90; the optional a, avg arguments of module PDFS).  Fields u(nx, ny, nz), x fastest; a gate is
// int8 with the same layout.
//
//   k_gate_levels           one thread per point, 8 bytes in and 1 byte out: the first n with a < thr(n), else igate_size.  The thresholds come in
//                           the kernel arguments and are put into LDS once per workgroup.
//   k_gate_flux             the quadrants of (a, v): 16 bytes in, 1 byte out.
//   k_gated_moments<V, NM>  the grid and the rows of k_pdf_hist / k_plane_partial: grid (ny, nchunks, nv), 256 threads, the workgroup (j, c, v)
//                           takes PDF_ROWS_PER_GROUP rows of k of plane j of field v; wave w takes the rows c R + w, + 4, ..; its lanes run
//                           along x, V = 2: 16-byte loads (nx even, every field 16-byte aligned), V = 1: 8-byte loads; four rows are requested
//                           before the first is used; the gate goes byte-wise.  A thread keeps acc[level][m] for COND_LEVELS_PER_LAUNCH levels
//                           g0 .. and NM moments in registers; a point adds gate == g ? a**m : 0.0 (adding +0.0 is exact: no branch), the
//                           powers formed once per point by the products of the runtime's square-and-multiply (powers<NM>,
//                           conditional_host.hpp).  Counts are 32-bit integers beside the sums.  Then the wave by __shfl_xor, the four waves
//                           through LDS in wave order, and thread 0 stores partial[v][c][j][level][m] and cnt[c][j][level].  More levels take
//                           more launches; without a gate every point has level 1.
//   k_gated_moments_final   sums the chunks of every (v, j, level, m) in chunk order into sums(ny, nm, nv, L), the counts into nsample(ny, L).
//                           Nothing is divided here: the one division per output and RAW_TO_CENTRAL are host arithmetic on ny nm nv L numbers.
//   k_cavg_sum<V, TWO>      the same grid and row order.  A fp64 sum per bin WITHOUT atomics: every wave owns a table [table][bin][column] of
//                           sums and of 32-bit counts in LDS (table: the plane's, the volume's).  Lane l owns column l % COLS and updates it by a
//                           plain read-add-write; where COLS < 64 the wave goes through its points in 64 / COLS phases and in phase p only the
//                           lanes with l / COLS == p act, so a slot has one writer at a time and a fixed order.  COLS = the largest power of two
//                           with which the tables fit (cavg_columns); where both tables do not fit even with one column the volume takes a
//                           launch of its own.  The bin is pdf_bin (pdfs_host.hpp), computed once for the sum and the count.  At the end the
//                           columns are summed in column order and the waves in wave order: psum, pcnt[v][c][j][table][bin], plain stores.
//                           TWO: the bin of (u, v) is vp nb1 + up with the v-interval of u-bin up (PDF2V2D).
//   k_cavg_planes           sums the chunks of every (v, j, bin) in chunk order, of the plane's table and of the volume's.
//   k_cavg_volume           sums the volume's plane parts in plane order.
//
// No global atomics, no float atomics, no workgroup that waits for or counts another: the order of every fp64 sum is a function of the shapes and
// the alignment alone, so a call repeats its bits.  nz = 1 and lines shorter than a wave are correct but slow, as in k_plane_partial.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <type_traits>

#include "conditional_host.hpp"
#include "kernels.hpp"
#include "profile.hpp"

#pragma clang fp contract(off)      // every multiply and add below stays as written

namespace tlab {
namespace {

constexpr int COND_THREADS = 256, COND_WAVES = COND_THREADS / 64, COND_ROWS_AHEAD = 4, COND_SLOTS = CAVG_LDS_BYTES / 12;
static_assert(COND_WAVES == CAVG_WAVES, "cavg_columns counts the waves of k_cavg_sum");

struct GateArgs {
    double thr[GATE_MAX_THRESHOLDS];
    const double *a;
    signed char *gate;
    long long n;
    int igate_size;
};

__global__ void __launch_bounds__(COND_THREADS) k_gate_levels(const GateArgs a) {
    __shared__ double thr[GATE_MAX_THRESHOLDS];
    for (int t = threadIdx.x; t < a.igate_size - 1; t += COND_THREADS) thr[t] = a.thr[t];
    __syncthreads();
    const long long stride = (long long)gridDim.x * COND_THREADS;
    for (long long i = (long long)blockIdx.x * COND_THREADS + threadIdx.x; i < a.n; i += stride) a.gate[i] = gate_level(a.a[i], thr, a.igate_size);
}

__global__ void __launch_bounds__(COND_THREADS) k_gate_flux(const double *__restrict__ a, const double *__restrict__ v, long long n,
                                                            signed char *__restrict__ gate) {
    const long long stride = (long long)gridDim.x * COND_THREADS;
    for (long long i = (long long)blockIdx.x * COND_THREADS + threadIdx.x; i < n; i += stride) gate[i] = gate_quadrant(a[i], v[i]);
}

// U rows (k, k + 4, ..) of one wave: fn(x, g) for every point, x[NF] its values in the NF fields, g its gate byte (1 without a gate)
template <int V, int U, int NF, class F>
__device__ __forceinline__ void cond_rows(const double *const *f, const signed char *g, size_t row0, size_t rstride, int nx, int lane, F &&fn) {
    using T = std::conditional_t<V == 2, double2, double>;
    for (int i = lane * V; i < nx; i += 64 * V) {
        T x[U][NF];
        signed char m[U][V];
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int c = 0; c < NF; ++c) x[u][c] = *reinterpret_cast<const T *>(f[c] + row0 + u * rstride + i);
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int e = 0; e < V; ++e) m[u][e] = g ? g[row0 + u * rstride + i + e] : (signed char)1;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            double y[NF];
            if constexpr (V == 2) {
#pragma unroll
                for (int c = 0; c < NF; ++c) y[c] = x[u][c].x;
                fn(y, (int)m[u][0]);
#pragma unroll
                for (int c = 0; c < NF; ++c) y[c] = x[u][c].y;
                fn(y, (int)m[u][1]);
            } else {
#pragma unroll
                for (int c = 0; c < NF; ++c) y[c] = x[u][c];
                fn(y, (int)m[u][0]);
            }
        }
    }
}

// the rows of workgroup (j, c), wave by wave
template <int V, int NF, class F>
__device__ __forceinline__ void cond_chunk(const double *const *f, const signed char *g, int nx, int ny, int nz, int j, int c, int wave, int lane,
                                           F &&fn) {
    constexpr int U = COND_ROWS_AHEAD;
    const int k1 = min(nz, (c + 1) * PDF_ROWS_PER_GROUP);
    const size_t plane = (size_t)nx * ny, rstride = COND_WAVES * plane;
    int k = c * PDF_ROWS_PER_GROUP + wave;
    for (; k + COND_WAVES * (U - 1) < k1; k += COND_WAVES * U) cond_rows<V, U, NF>(f, g, (size_t)k * plane + (size_t)j * nx, rstride, nx, lane, fn);
    for (; k < k1; k += COND_WAVES) cond_rows<V, 1, NF>(f, g, (size_t)k * plane + (size_t)j * nx, rstride, nx, lane, fn);
}

struct MomArgs {
    const double *f[PDF_FIELDS_PER_LAUNCH];
    const signed char *gate;
    double *partial;      // [nv][nchunks][ny][COND_LEVELS_PER_LAUNCH][NM]
    unsigned *cnt;        // [nchunks][ny][COND_LEVELS_PER_LAUNCH]
    int nx, ny, nz, g0;
};

template <int V, int NM>
__global__ void __launch_bounds__(COND_THREADS) k_gated_moments(const MomArgs a) {
    constexpr int LG = COND_LEVELS_PER_LAUNCH;
    __shared__ double red[COND_WAVES][LG * NM];
    __shared__ unsigned redn[COND_WAVES][LG];
    const int j = blockIdx.x, c = blockIdx.y, v = blockIdx.z, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double acc[LG][NM];
    unsigned n[LG];
#pragma unroll
    for (int l = 0; l < LG; ++l) {
        n[l] = 0u;
#pragma unroll
        for (int m = 0; m < NM; ++m) acc[l][m] = 0.0;
    }
    const double *f[1] = {a.f[v]};
    const int g0 = a.g0;
    cond_chunk<V, 1>(f, a.gate, a.nx, a.ny, a.nz, j, c, wave, lane, [&](const double *x, int g) {
        double p[NM];
        powers<NM>(x[0], p);
#pragma unroll
        for (int l = 0; l < LG; ++l) {
            const bool on = g == g0 + l;
            n[l] += on ? 1u : 0u;
#pragma unroll
            for (int m = 0; m < NM; ++m) acc[l][m] += on ? p[m] : 0.0;
        }
    });
#pragma unroll
    for (int l = 0; l < LG; ++l) {
        unsigned s = n[l];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
        if (lane == 0) redn[wave][l] = s;
#pragma unroll
        for (int m = 0; m < NM; ++m) {
            double t = acc[l][m];
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) t += __shfl_xor(t, d, 64);
            if (lane == 0) red[wave][l * NM + m] = t;
        }
    }
    __syncthreads();
    if (threadIdx.x < LG * NM) {
        double s = red[0][threadIdx.x];
        for (int w = 1; w < COND_WAVES; ++w) s += red[w][threadIdx.x];
        a.partial[((((size_t)v * gridDim.y + c) * a.ny + j) * LG) * NM + threadIdx.x] = s;
    }
    if (v == 0 && threadIdx.x < LG) {
        unsigned s = redn[0][threadIdx.x];
        for (int w = 1; w < COND_WAVES; ++w) s += redn[w][threadIdx.x];
        a.cnt[((size_t)c * a.ny + j) * LG + threadIdx.x] = s;
    }
}

// sums(ny, nm, nvt, L), nsample(ny, L) in Fortran order; this launch holds the fields v0 .. v0 + nv - 1 and the levels g0 .. (0-based l0 ..)
__global__ void __launch_bounds__(COND_THREADS) k_gated_moments_final(const double *__restrict__ partial, const unsigned *__restrict__ cnt, int nchunks,
                                                                      int ny, int nv, int NM, int nm, int v0, int nvt, int l0, int L,
                                                                      double *__restrict__ sums, long long *__restrict__ nsample) {
    constexpr int LG = COND_LEVELS_PER_LAUNCH;
    const long long t = (long long)blockIdx.x * COND_THREADS + threadIdx.x;
    if (t >= (long long)nv * ny * LG * NM) return;
    const int m = (int)(t % NM), l = (int)(t / NM % LG), j = (int)(t / (NM * LG) % ny), v = (int)(t / ((long long)NM * LG * ny));
    if (m >= nm || l0 + l >= L) return;
    double s = 0.0;
    for (int c = 0; c < nchunks; ++c) s += partial[((((size_t)v * nchunks + c) * ny + j) * LG + l) * NM + m];
    sums[(((size_t)(l0 + l) * nvt + v0 + v) * nm + m) * ny + j] = s;
    if (v == 0 && v0 == 0 && m == 0) {
        long long ns = 0;
        for (int c = 0; c < nchunks; ++c) ns += cnt[((size_t)c * ny + j) * LG + l];
        nsample[(size_t)(l0 + l) * ny + j] = ns;
    }
}

struct CavgArgs {
    const double *f[PDF_FIELDS_PER_LAUNCH];
    const double *v2, *a;              // TWO: the second variable; the field that is averaged
    const signed char *gate;
    const double *iv;                  // [nv][ny + 1][2] = (umin, ustep) of every plane and of the volume
    const double *viv;                 // TWO: [ny + 1][nb1][2] = (vmin, vstep) of every u-bin
    double *psum;                      // [nv][nchunks][ny][2][nbins]
    unsigned *pcnt;                    // the same
    int nx, ny, nz, igate, nbins, nb1, nb2, cols, tab0, ntab;
    unsigned ext_mask;                 // bit v: field v has an external interval
};

template <int V, bool TWO>
__global__ void __launch_bounds__(COND_THREADS) k_cavg_sum(const CavgArgs a) {
    __shared__ double lsum[COND_SLOTS];        // [wave][ntab][nbins][cols]
    __shared__ unsigned lcnt[COND_SLOTS];
    constexpr int NF = TWO ? 3 : 2;
    const int j = blockIdx.x, c = blockIdx.y, v = blockIdx.z, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int nb = a.nbins, cols = a.cols, ntab = a.ntab, phases = 64 / cols, col = lane & (cols - 1), phase = lane / cols;
    for (int t = threadIdx.x; t < COND_WAVES * ntab * nb * cols; t += COND_THREADS) { lsum[t] = 0.0; lcnt[t] = 0u; }
    __syncthreads();
    const bool ext = (a.ext_mask >> v) & 1u;
    const double *iv = a.iv + (size_t)v * (a.ny + 1) * 2;
    const double *f[NF];
    f[0] = a.f[v];
    if constexpr (TWO) f[1] = a.v2;
    f[NF - 1] = a.a;
    const int igate = a.igate, base = wave * ntab * nb * cols + col;
    int row[2];                  // the plane of the intervals of table t: j, or ny for the volume
    double umin[2], ustep[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        row[t] = a.tab0 + t == 0 ? j : a.ny;
        umin[t] = iv[2 * row[t]];
        ustep[t] = iv[2 * row[t] + 1];
    }
    cond_chunk<V, NF>(f, a.igate != 0 ? a.gate : nullptr, a.nx, a.ny, a.nz, j, c, wave, lane, [&](const double *x, int g) {
        int bin[2] = {-1, -1};
        if (igate == 0 || g == igate) {
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                if (t >= ntab) break;
                int b = pdf_bin(x[0], umin[t], ustep[t], TWO ? a.nb1 : nb, ext);
                if constexpr (TWO) {
                    if ((unsigned)b < (unsigned)a.nb1) {
                        const double *w = a.viv + ((size_t)row[t] * a.nb1 + b) * 2;
                        const int vp = pdf_bin(x[1], w[0], w[1], a.nb2, false);
                        b = (unsigned)vp < (unsigned)a.nb2 ? vp * a.nb1 + b : -1;
                    }
                }
                bin[t] = (unsigned)b < (unsigned)nb ? b : -1;
            }
        }
        // One writer per slot at a time, in the order of the phases.  What this relies on: (1) the hardware -- a wave issues its LDS instructions in
        // program order and the LDS completes those of one wave in that order, so the read-add-write of phase p is done before that of phase
        // p + 1 reads; (2) the compiler -- for one THREAD the loop is a single conditional update, and nothing in C++ says that other lanes touch
        // the same slot, so the loop must be kept as `phases` separate steps: the fence (wavefront scope: no instruction is emitted) forbids
        // moving an LDS access from one iteration into another, the wave barrier forbids rescheduling across it.  Were the loop ever collapsed,
        // lanes of different phases would add to one slot in one instruction and updates would be lost: the counts and the exact-data sums of
        // tests/test_gpu_conditional.py, which must equal the reference's in every word, fail then.
        for (int p = 0; p < phases; ++p) {
            if (p == phase) {
#pragma unroll
                for (int t = 0; t < 2; ++t)
                    if (bin[t] >= 0) {
                        const int s = base + (t * nb + bin[t]) * cols;
                        lsum[s] = lsum[s] + x[NF - 1];
                        lcnt[s] = lcnt[s] + 1u;
                    }
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
    });
    __syncthreads();
    const size_t out = ((((size_t)v * gridDim.y + c) * a.ny + j) * 2 + a.tab0) * nb;
    for (int t = threadIdx.x; t < ntab * nb; t += COND_THREADS) {      // t = table * nb + bin: the columns in column order, the waves in wave order
        double s = 0.0;
        unsigned n = 0u;
        for (int w = 0; w < COND_WAVES; ++w) {
            const int s0 = (w * ntab * nb + t) * cols;
            double sw = lsum[s0];
            for (int q = 1; q < cols; ++q) sw += lsum[s0 + q];
            s += sw;
            for (int q = 0; q < cols; ++q) n += lcnt[s0 + q];
        }
        a.psum[out + t] = s;
        a.pcnt[out + t] = n;
    }
}

// sum, cnt[v][j][b] = the chunks of plane j in chunk order; volsum, volcnt[v][j][b] = plane j's part of the volume's
__global__ void __launch_bounds__(COND_THREADS) k_cavg_planes(const double *__restrict__ psum, const unsigned *__restrict__ pcnt, int nchunks, int ny,
                                                              int nb, double *__restrict__ sum, double *__restrict__ cnt,
                                                              double *__restrict__ volsum, unsigned long long *__restrict__ volcnt) {
    const int j = blockIdx.x, v = blockIdx.y;
    for (int b = threadIdx.x; b < nb; b += COND_THREADS) {
        double s = 0.0, sv = 0.0;
        unsigned long long n = 0ull, nv = 0ull;
        for (int c = 0; c < nchunks; ++c) {
            const size_t p = ((((size_t)v * nchunks + c) * ny + j) * 2) * nb + b;
            s += psum[p];
            n += pcnt[p];
            if (ny > 1) { sv += psum[p + nb]; nv += pcnt[p + nb]; }
        }
        sum[((size_t)v * (ny + 1) + j) * nb + b] = s;
        cnt[((size_t)v * (ny + 1) + j) * nb + b] = (double)n;
        volsum[((size_t)v * ny + j) * nb + b] = sv;
        volcnt[((size_t)v * ny + j) * nb + b] = nv;
    }
}

// sum, cnt[v][ny][b] = the planes' parts in plane order: grid (ceil(nb / 256), nv), one thread per bin
__global__ void __launch_bounds__(COND_THREADS) k_cavg_volume(const double *__restrict__ volsum, const unsigned long long *__restrict__ volcnt, int ny,
                                                              int nb, double *__restrict__ sum, double *__restrict__ cnt) {
    const int v = blockIdx.y, b = blockIdx.x * COND_THREADS + threadIdx.x;
    if (b >= nb) return;
    double s = 0.0;
    unsigned long long n = 0ull;
    for (int j = 0; j < ny; ++j) {
        s += volsum[((size_t)v * ny + j) * nb + b];
        n += volcnt[((size_t)v * ny + j) * nb + b];
    }
    sum[((size_t)v * (ny + 1) + ny) * nb + b] = s;
    cnt[((size_t)v * (ny + 1) + ny) * nb + b] = (double)n;
}

bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

// the checks every launch on a box shares; vec: 16-byte loads
bool cond_box(const PdfFields &F, bool &vec) {
    if (F.nx < 1 || F.ny < 1 || F.nz < 1 || F.nv < 1 || F.nv > PDF_FIELDS_PER_LAUNCH || pdf_chunks(F.nz) > 65535) return false;
    vec = F.nx % 2 == 0;
    for (int i = 0; i < F.nv; ++i) {
        if (!F.f[i]) return false;
        vec = vec && aligned16(F.f[i]);
    }
    return true;
}

template <int NM>
void moments_launch(bool vec, dim3 grid, hipStream_t st, const MomArgs &a) {
    if (vec) hipLaunchKernelGGL((k_gated_moments<2, NM>), grid, dim3(COND_THREADS), 0, st, a);
    else hipLaunchKernelGGL((k_gated_moments<1, NM>), grid, dim3(COND_THREADS), 0, st, a);
}

}  // namespace

int gated_moments_width(int nm) { return nm <= 2 ? 2 : nm <= 4 ? 4 : COND_MAX_MOMENTS; }

hipError_t launch_gate_levels(const double *a, long long n, int igate_size, const double *thr, signed char *gate, hipStream_t st) {
    if (!a || !gate || n < 1 || igate_size < 1 || igate_size > GATE_MAX_LEVELS || (igate_size > 1 && !thr)) return hipErrorInvalidValue;
    GateArgs g{};
    for (int t = 0; t < igate_size - 1; ++t) g.thr[t] = thr[t];
    g.a = a; g.gate = gate; g.n = n; g.igate_size = igate_size;
    const long long nblocks = std::min<long long>((n + COND_THREADS - 1) / COND_THREADS, 65536);
    ProfScope ps("k_gate_levels", st, 9.0 * (double)n);
    hipLaunchKernelGGL(k_gate_levels, dim3((unsigned)nblocks), dim3(COND_THREADS), 0, st, g);
    return hipGetLastError();
}

hipError_t launch_gate_flux(const double *a, const double *v, long long n, signed char *gate, hipStream_t st) {
    if (!a || !v || !gate || n < 1) return hipErrorInvalidValue;
    const long long nblocks = std::min<long long>((n + COND_THREADS - 1) / COND_THREADS, 65536);
    ProfScope ps("k_gate_flux", st, 17.0 * (double)n);
    hipLaunchKernelGGL(k_gate_flux, dim3((unsigned)nblocks), dim3(COND_THREADS), 0, st, a, v, n, gate);
    return hipGetLastError();
}

hipError_t launch_gated_moments(const PdfFields &F, int nm, int g0, int L, int v0, int nvt, double *partial, unsigned *cnt, double *sums,
                                long long *nsample, hipStream_t st) {
    bool vec = false;
    if (!cond_box(F, vec) || nm < 1 || nm > COND_MAX_MOMENTS || g0 < 1 || L < 1 || g0 > L || v0 < 0 || v0 + F.nv > nvt || !partial || !cnt || !sums ||
        !nsample)
        return hipErrorInvalidValue;
    MomArgs a{};
    for (int i = 0; i < F.nv; ++i) a.f[i] = F.f[i];
    a.gate = F.gate; a.partial = partial; a.cnt = cnt; a.nx = F.nx; a.ny = F.ny; a.nz = F.nz; a.g0 = g0;
    const int nchunks = pdf_chunks(F.nz), NM = gated_moments_width(nm);
    const dim3 grid((unsigned)F.ny, (unsigned)nchunks, (unsigned)F.nv);
    {
        ProfScope ps("k_gated_moments", st, (double)F.nx * F.ny * (double)F.nz * F.nv * (8.0 + (F.gate ? 1.0 : 0.0)));
        if (NM == 2) moments_launch<2>(vec, grid, st, a);
        else if (NM == 4) moments_launch<4>(vec, grid, st, a);
        else moments_launch<COND_MAX_MOMENTS>(vec, grid, st, a);
    }
    const long long nt = (long long)F.nv * F.ny * COND_LEVELS_PER_LAUNCH * NM;
    hipLaunchKernelGGL(k_gated_moments_final, dim3((unsigned)((nt + COND_THREADS - 1) / COND_THREADS)), dim3(COND_THREADS), 0, st, partial, cnt, nchunks,
                       F.ny, F.nv, NM, nm, v0, nvt, g0 - 1, L, sums, nsample);
    return hipGetLastError();
}

hipError_t launch_cavg_sum(const PdfFields &F, const double *v2, const double *a, int nb1, int nb2, unsigned ext_mask, const double *iv,
                           const double *viv, double *psum, unsigned *pcnt, double *volsum, unsigned long long *volcnt, double *sum, double *cnt,
                           hipStream_t st) {
    bool vec = false;
    const bool two = nb2 > 0;
    const long long nbl = (long long)nb1 * (two ? nb2 : 1);
    if (!cond_box(F, vec) || (F.igate != 0 && !F.gate) || !a || nb1 < 1 || nb2 < 0 || nbl > CAVG_MAX_BINS || (two && (!v2 || !viv || F.nv != 1)) || !iv ||
        !psum || !pcnt || !volsum || !volcnt || !sum || !cnt)
        return hipErrorInvalidValue;
    vec = vec && aligned16(a) && (!two || aligned16(v2));
    CavgArgs k{};
    for (int i = 0; i < F.nv; ++i) k.f[i] = F.f[i];
    k.v2 = v2; k.a = a; k.gate = F.gate; k.iv = iv; k.viv = viv; k.psum = psum; k.pcnt = pcnt;
    k.nx = F.nx; k.ny = F.ny; k.nz = F.nz; k.igate = F.igate; k.nbins = (int)nbl; k.nb1 = nb1; k.nb2 = nb2; k.ext_mask = ext_mask;
    const int nchunks = pdf_chunks(F.nz), want = F.ny > 1 ? 2 : 1;
    const int per = cavg_columns(k.nbins, want) >= 1 ? want : 1;      // tables per launch
    if (cavg_columns(k.nbins, per) < 1) return hipErrorInvalidValue;
    const dim3 grid((unsigned)F.ny, (unsigned)nchunks, (unsigned)F.nv), block(COND_THREADS);
    for (int tab0 = 0; tab0 < want; tab0 += per) {
        k.tab0 = tab0; k.ntab = per; k.cols = cavg_columns(k.nbins, per);
        ProfScope ps("k_cavg_sum", st, (double)F.nx * F.ny * (double)F.nz * (8.0 * (F.nv + (two ? 2 : 1)) + (F.igate != 0 ? 1.0 : 0.0)));
        if (two) {
            if (vec) hipLaunchKernelGGL((k_cavg_sum<2, true>), grid, block, 0, st, k);
            else hipLaunchKernelGGL((k_cavg_sum<1, true>), grid, block, 0, st, k);
        } else {
            if (vec) hipLaunchKernelGGL((k_cavg_sum<2, false>), grid, block, 0, st, k);
            else hipLaunchKernelGGL((k_cavg_sum<1, false>), grid, block, 0, st, k);
        }
    }
    hipLaunchKernelGGL(k_cavg_planes, dim3((unsigned)F.ny, (unsigned)F.nv), block, 0, st, psum, pcnt, nchunks, F.ny, k.nbins, sum, cnt, volsum, volcnt);
    if (F.ny > 1)
        hipLaunchKernelGGL(k_cavg_volume, dim3((unsigned)((k.nbins + COND_THREADS - 1) / COND_THREADS), (unsigned)F.nv), block, 0, st, volsum, volcnt, F.ny,
                           k.nbins, sum, cnt);
    return hipGetLastError();
}

}  // namespace tlab

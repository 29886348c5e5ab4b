// Plane PDFs on the device: the histograms of PDF1V_N (statistics/pdf.f90:14-119) over module PDFS (utils/pdfs.f90: PDF1V2D :28-111, PDF1V2D1G
// :121-210) for every field, every plane j and the whole volume in THREE streaming passes (min/max, histogram, histogram on the analysed interval)
// instead of four strided passes per field and plane.  Fields u(nx, ny, nz), x fastest; a gate is int8 with the same layout.
//
//   k_pdf_minmax<V, GATE>   grid (ny, nchunks, nv), 256 threads: the workgroup (j, c, v) takes the rows k of chunk c (PDF_ROWS_PER_GROUP rows) of
//                           plane j of field v.  Wave w takes the rows c R + w, + 4, ..; its lanes run along x, V = 2: 16-byte loads (nx even, the
//                           field 16-byte aligned), V = 1: 8-byte loads; four rows are requested before the first is used.  Min and max by
//                           compare-and-select, the wave by __shfl_xor, the four waves through LDS; thread 0 stores partial[v][c][j][2].  Gated:
//                           only points with gate == igate take part, and both start from big_wp = 1e20 / -big_wp as in PDF1V2D1G.
//   k_pdf_minmax_final      grid (nv): the chunks of every plane, then the planes to the volume (plane ny).  Order-free: exact.
//   k_pdf_hist<V, GATE>     the same grid and row order.  A point is binned (pdf_bin, pdfs_host.hpp) into the plane's table with the plane's
//                           (umin, ustep) and, where the field's bit of vol_mask is set, into the volume's table with the volume's.  Counters are
//                           32-bit integers in LDS, REP replicas of each table: lane l adds to replica l % REP at tab[bin REP + l % REP], so with
//                           REP = 32 every lane of a half wave has a bank of its own whatever the data (a constant field: lanes l and l + 32
//                           meet, nothing else).  REP = the largest power of two <= 32 with 2 nbins REP <= PDF_LDS_WORDS.  The index is checked
//                           against [0, nbins) before the atomic.  At the end the replicas are summed and the counts of the workgroup go to
//                           cnt[v][c][j][table][bin] with plain vector stores.
//   k_pdf_hist_planes       sums the chunks of each (v, j, bin) into a double, and the volume's partial of plane j into a 64-bit integer (from
//                           the plane's own counts where the volume was not binned: with one external interval for all planes the volume
//                           histogram IS the sum of the planes')
//   k_pdf_hist_volume       sums those over the planes.
//   k_gate_threshold        gate = a > thr ? 1 : 0 (the gate of dns_statistics.f90:106-110).
//   k_gate_count            INTER1V2D for every plane and level in one pass over the gate (further down), k_gate_count_final its chunks.
//
// No global atomics, no float atomics, no workgroup that waits for or counts another: integer counts are exact in any order, so a call repeats
// its bits, and they are the reference's as long as a count stays below 2^53 (a chunk of one plane below 2^32).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <type_traits>

#include "kernels.hpp"
#include "pdfs_host.hpp"
#include "profile.hpp"

#pragma clang fp contract(off)      // every operation below stays as written

namespace tlab {
namespace {

constexpr int PDF_THREADS = 256, PDF_WAVES = PDF_THREADS / 64, PDF_ROWS_AHEAD = 4;

struct PdfArgs {
    const double *f[PDF_FIELDS_PER_LAUNCH];
    const signed char *gate;
    const double *iv;                  // k_pdf_hist: [nv][ny + 1][2] = (umin, ustep) of every plane and of the volume
    double *partial;                   // k_pdf_minmax: [nv][nchunks][ny][2]
    unsigned *cnt;                     // k_pdf_hist: [nv][nchunks][ny][ntab][nbins]
    int nx, ny, nz, igate, nbins, rep, ntab;
    unsigned ext_mask, vol_mask;       // bit v: field v has an external interval / bins the volume's table too
};

// U rows (k, k + 4, ..) of one wave: fn(x, y) for every point that takes part, x of field f0, y of field f1 (NF = 2; 0.0 otherwise)
template <int V, int U, int NF, bool GATE, class F>
__device__ __forceinline__ void pdf_rows(const double *f0, const double *f1, const signed char *g, int igate, size_t row0, size_t rstride, int nx,
                                         int lane, F &&fn) {
    using T = std::conditional_t<V == 2, double2, double>;
    for (int i = lane * V; i < nx; i += 64 * V) {
        T x[U], y[U];
        signed char m[U][V];
#pragma unroll
        for (int u = 0; u < U; ++u) x[u] = *reinterpret_cast<const T *>(f0 + row0 + u * rstride + i);
        if constexpr (NF == 2) {
#pragma unroll
            for (int u = 0; u < U; ++u) y[u] = *reinterpret_cast<const T *>(f1 + row0 + u * rstride + i);
        }
        if constexpr (GATE) {
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int e = 0; e < V; ++e) m[u][e] = g[row0 + u * rstride + i + e];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if constexpr (V == 2) {
                if (!GATE || m[u][0] == igate) fn(x[u].x, NF == 2 ? y[u].x : 0.0);
                if (!GATE || m[u][1] == igate) fn(x[u].y, NF == 2 ? y[u].y : 0.0);
            } else {
                if (!GATE || m[u][0] == igate) fn(x[u], NF == 2 ? y[u] : 0.0);
            }
        }
    }
}

// the rows of workgroup (j, c), wave by wave
template <int V, int NF, bool GATE, class F>
__device__ __forceinline__ void pdf_chunk(const PdfArgs &a, const double *f0, const double *f1, int j, int c, int wave, int lane, F &&fn) {
    constexpr int U = PDF_ROWS_AHEAD;
    const int k1 = min(a.nz, (c + 1) * PDF_ROWS_PER_GROUP);
    const size_t plane = (size_t)a.nx * a.ny, rstride = PDF_WAVES * plane;
    int k = c * PDF_ROWS_PER_GROUP + wave;
    for (; k + PDF_WAVES * (U - 1) < k1; k += PDF_WAVES * U)
        pdf_rows<V, U, NF, GATE>(f0, f1, a.gate, a.igate, (size_t)k * plane + (size_t)j * a.nx, rstride, a.nx, lane, fn);
    for (; k < k1; k += PDF_WAVES) pdf_rows<V, 1, NF, GATE>(f0, f1, a.gate, a.igate, (size_t)k * plane + (size_t)j * a.nx, rstride, a.nx, lane, fn);
}

template <int V, bool GATE>
__global__ void __launch_bounds__(PDF_THREADS) k_pdf_minmax(const PdfArgs a) {
    __shared__ double red[PDF_WAVES][2];
    const int j = blockIdx.x, c = blockIdx.y, v = blockIdx.z, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double mn = GATE ? PDF_BIG : __builtin_huge_val(), mx = GATE ? -PDF_BIG : -__builtin_huge_val();
    pdf_chunk<V, 1, GATE>(a, a.f[v], nullptr, j, c, wave, lane, [&](double x, double) {
        mn = x < mn ? x : mn;
        mx = x > mx ? x : mx;
    });
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const double on = __shfl_xor(mn, d, 64), ox = __shfl_xor(mx, d, 64);
        mn = on < mn ? on : mn;
        mx = ox > mx ? ox : mx;
    }
    if (lane == 0) { red[wave][0] = mn; red[wave][1] = mx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < PDF_WAVES; ++w) {
            mn = red[w][0] < mn ? red[w][0] : mn;
            mx = red[w][1] > mx ? red[w][1] : mx;
        }
        double *out = a.partial + (((size_t)v * gridDim.y + c) * a.ny + j) * 2;
        out[0] = mn;
        out[1] = mx;
    }
}

// mm[v][j][2], j < ny: the chunks of plane j; mm[v][ny][2]: the planes
__global__ void __launch_bounds__(PDF_THREADS) k_pdf_minmax_final(const double *__restrict__ partial, int nchunks, int ny, double *__restrict__ mm) {
    __shared__ double red[PDF_WAVES][2];
    const int v = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double vmn = __builtin_huge_val(), vmx = -__builtin_huge_val();
    for (int j = threadIdx.x; j < ny; j += PDF_THREADS) {
        const double *p = partial + ((size_t)v * nchunks * ny + j) * 2;
        double mn = p[0], mx = p[1];
        for (int c = 1; c < nchunks; ++c) {
            const double *q = p + (size_t)c * ny * 2;
            mn = q[0] < mn ? q[0] : mn;
            mx = q[1] > mx ? q[1] : mx;
        }
        double *o = mm + ((size_t)v * (ny + 1) + j) * 2;
        o[0] = mn;
        o[1] = mx;
        vmn = mn < vmn ? mn : vmn;
        vmx = mx > vmx ? mx : vmx;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const double on = __shfl_xor(vmn, d, 64), ox = __shfl_xor(vmx, d, 64);
        vmn = on < vmn ? on : vmn;
        vmx = ox > vmx ? ox : vmx;
    }
    if (lane == 0) { red[wave][0] = vmn; red[wave][1] = vmx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < PDF_WAVES; ++w) {
            vmn = red[w][0] < vmn ? red[w][0] : vmn;
            vmx = red[w][1] > vmx ? red[w][1] : vmx;
        }
        double *o = mm + ((size_t)v * (ny + 1) + ny) * 2;
        o[0] = vmn;
        o[1] = vmx;
    }
}

template <int V, bool GATE>
__global__ void __launch_bounds__(PDF_THREADS) k_pdf_hist(const PdfArgs a) {
    __shared__ unsigned tab[PDF_LDS_WORDS];      // [ntab][nbins][rep]
    const int j = blockIdx.x, c = blockIdx.y, v = blockIdx.z, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int nb = a.nbins, rep = a.rep, nw = nb * rep, rl = lane & (rep - 1);
    const bool ext = (a.ext_mask >> v) & 1u, vol = (a.vol_mask >> v) & 1u;
    for (int t = threadIdx.x; t < a.ntab * nw; t += PDF_THREADS) tab[t] = 0u;
    __syncthreads();
    const double *iv = a.iv + (size_t)v * (a.ny + 1) * 2;
    const double pmin = iv[2 * j], pstep = iv[2 * j + 1], vmin = iv[2 * a.ny], vstep = iv[2 * a.ny + 1];
    pdf_chunk<V, 1, GATE>(a, a.f[v], nullptr, j, c, wave, lane, [&](double x, double) {
        const int b = pdf_bin(x, pmin, pstep, nb, ext);
        if ((unsigned)b < (unsigned)nb) atomicAdd(&tab[b * rep + rl], 1u);
        if (vol) {
            const int bv = pdf_bin(x, vmin, vstep, nb, ext);
            if ((unsigned)bv < (unsigned)nb) atomicAdd(&tab[nw + bv * rep + rl], 1u);
        }
    });
    __syncthreads();
    unsigned *out = a.cnt + (((size_t)v * gridDim.y + c) * a.ny + j) * a.ntab * nb;
    for (int t = threadIdx.x; t < a.ntab * nb; t += PDF_THREADS) {      // t = table * nb + bin: its replicas lie at tab[t rep ..]
        unsigned s = 0u;
        for (int r = 0; r < rep; ++r) s += tab[t * rep + ((r + threadIdx.x) & (rep - 1))];      // (rotated: the threads start on different banks)
        out[t] = s;
    }
}

// pdf[v][j][b] = the chunks of plane j; volpart[v][j][b] = plane j's part of the volume's count
__global__ void __launch_bounds__(PDF_THREADS) k_pdf_hist_planes(const unsigned *__restrict__ cnt, int nchunks, int ny, int ntab, int nb,
                                                                 unsigned vol_mask, double *__restrict__ pdf,
                                                                 unsigned long long *__restrict__ volpart) {
    const int j = blockIdx.x, v = blockIdx.y;
    const bool vol = (vol_mask >> v) & 1u;
    for (int b = threadIdx.x; b < nb; b += PDF_THREADS) {
        unsigned long long s = 0ull, sv = 0ull;
        for (int c = 0; c < nchunks; ++c) {
            const unsigned *p = cnt + (((size_t)v * nchunks + c) * ny + j) * ntab * nb;
            s += p[b];
            if (vol) sv += p[nb + b];
        }
        pdf[((size_t)v * (ny + 1) + j) * nb + b] = (double)s;
        volpart[((size_t)v * ny + j) * nb + b] = vol ? sv : s;
    }
}

// pdf[v][ny][b] = the sum of volpart[v][.][b]: grid (ceil(nb / 64), nv); lane = bin, the waves share the planes
__global__ void __launch_bounds__(PDF_THREADS) k_pdf_hist_volume(const unsigned long long *__restrict__ volpart, int ny, int nb, double *__restrict__ pdf) {
    __shared__ unsigned long long red[PDF_WAVES][64];
    const int v = blockIdx.y, wave = threadIdx.x >> 6, lane = threadIdx.x & 63, b = blockIdx.x * 64 + lane;
    unsigned long long s = 0ull;
    if (b < nb)
        for (int j = wave; j < ny; j += PDF_WAVES) s += volpart[((size_t)v * ny + j) * nb + b];
    red[wave][lane] = s;
    __syncthreads();
    if (wave == 0 && b < nb) {
        for (int w = 1; w < PDF_WAVES; ++w) s += red[w][lane];
        pdf[((size_t)v * (ny + 1) + ny) * nb + b] = (double)s;
    }
}

// ---- PDF2V2D (utils/pdfs.f90:215-322): the joint histogram of (u, v) -----------------------------------------------------------------------------
// an order-preserving 64-bit key of a double (no NaN): larger double <=> larger key
__device__ __forceinline__ unsigned long long pdf_key(double x) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(x);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double pdf_unkey(unsigned long long k) {
    return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}

// k_pdf2v_range: grid (ny, nchunks).  The u-bin of a point (the plane's interval, and the volume's) selects an entry of the table of keys in LDS,
// [2 tables][nb1][min, max]; 64-bit integer LDS atomics (min / max of the key), issued only where the value improves what the entry holds -- after
// the first rows almost no point does, so equal bins in a wave do not serialise.  The entries start from big_wp / -big_wp as in the reference.
template <int V>
__global__ void __launch_bounds__(PDF_THREADS) k_pdf2v_range(const PdfArgs a) {
    __shared__ unsigned long long key[PDF_LDS_WORDS / 2];      // [ntab][nb1][2]
    const int j = blockIdx.x, c = blockIdx.y, wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nb = a.nbins;
    const unsigned long long kmin0 = pdf_key(PDF_BIG), kmax0 = pdf_key(-PDF_BIG);
    for (int t = threadIdx.x; t < a.ntab * nb * 2; t += PDF_THREADS) key[t] = (t & 1) ? kmax0 : kmin0;
    __syncthreads();
    const double pmin = a.iv[2 * j], pstep = a.iv[2 * j + 1], vmin = a.iv[2 * a.ny], vstep = a.iv[2 * a.ny + 1];
    const bool vol = a.ntab == 2;
    pdf_chunk<V, 2, false>(a, a.f[0], a.f[1], j, c, wave, lane, [&](double x, double y) {
        const unsigned long long k = pdf_key(y);
        const int b = pdf_bin(x, pmin, pstep, nb, false);
        if ((unsigned)b < (unsigned)nb) {
            if (k < key[2 * b]) atomicMin(&key[2 * b], k);
            if (k > key[2 * b + 1]) atomicMax(&key[2 * b + 1], k);
        }
        if (vol) {
            const int bv = pdf_bin(x, vmin, vstep, nb, false);
            if ((unsigned)bv < (unsigned)nb) {
                if (k < key[2 * (nb + bv)]) atomicMin(&key[2 * (nb + bv)], k);
                if (k > key[2 * (nb + bv) + 1]) atomicMax(&key[2 * (nb + bv) + 1], k);
            }
        }
    });
    __syncthreads();
    double *out = a.partial + ((size_t)c * a.ny + j) * a.ntab * nb * 2;
    for (int t = threadIdx.x; t < a.ntab * nb * 2; t += PDF_THREADS) out[t] = pdf_unkey(key[t]);
}

// rng[j][b][2] = the chunks of plane j; volpart[j][b][2] = plane j's part of the volume's (ntab = 2)
__global__ void __launch_bounds__(PDF_THREADS) k_pdf2v_range_planes(const double *__restrict__ partial, int nchunks, int ny, int ntab, int nb,
                                                                    double *__restrict__ rng, double *__restrict__ volpart) {
    const int j = blockIdx.x;
    for (int t = threadIdx.x; t < ntab * nb * 2; t += PDF_THREADS) {
        double r = partial[(size_t)j * ntab * nb * 2 + t];
        for (int c = 1; c < nchunks; ++c) {
            const double p = partial[((size_t)c * ny + j) * ntab * nb * 2 + t];
            r = (t & 1) ? (p > r ? p : r) : (p < r ? p : r);
        }
        if (t < nb * 2) rng[(size_t)j * nb * 2 + t] = r;
        else volpart[(size_t)j * nb * 2 + (t - nb * 2)] = r;
    }
}

// rng[ny][b][2] = the planes' parts: grid (ceil(2 nb1 / 64)); lane = entry, the waves share the planes
__global__ void __launch_bounds__(PDF_THREADS) k_pdf2v_range_volume(const double *__restrict__ volpart, int ny, int nb, double *__restrict__ rng) {
    __shared__ double red[PDF_WAVES][64];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, t = blockIdx.x * 64 + lane;
    const bool mx = t & 1;
    double r = mx ? -PDF_BIG : PDF_BIG;
    if (t < nb * 2)
        for (int j = wave; j < ny; j += PDF_WAVES) {
            const double p = volpart[(size_t)j * nb * 2 + t];
            r = mx ? (p > r ? p : r) : (p < r ? p : r);
        }
    red[wave][lane] = r;
    __syncthreads();
    if (wave == 0 && t < nb * 2) {
        for (int w = 1; w < PDF_WAVES; ++w) {
            const double p = red[w][lane];
            r = mx ? (p > r ? p : r) : (p < r ? p : r);
        }
        rng[(size_t)ny * nb * 2 + t] = r;
    }
}

// k_pdf2v_hist: as k_pdf_hist with the bin (up, vp) at vp nb1 + up; (vmin, vstep) of u-bin up from viv [ny + 1][nb1][2] (cached global loads)
template <int V>
__global__ void __launch_bounds__(PDF_THREADS) k_pdf2v_hist(const PdfArgs a, const double *__restrict__ viv, int nb1, int nb2) {
    __shared__ unsigned tab[PDF_LDS_WORDS];      // [ntab][nb1 nb2][rep]
    const int j = blockIdx.x, c = blockIdx.y, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int nb = a.nbins, rep = a.rep, nw = nb * rep, rl = lane & (rep - 1);
    for (int t = threadIdx.x; t < a.ntab * nw; t += PDF_THREADS) tab[t] = 0u;
    __syncthreads();
    const double pmin = a.iv[2 * j], pstep = a.iv[2 * j + 1], vmin = a.iv[2 * a.ny], vstep = a.iv[2 * a.ny + 1];
    const double *pv = viv + (size_t)j * nb1 * 2, *vv = viv + (size_t)a.ny * nb1 * 2;
    const bool vol = a.ntab == 2;
    pdf_chunk<V, 2, false>(a, a.f[0], a.f[1], j, c, wave, lane, [&](double x, double y) {
        const int up = pdf_bin(x, pmin, pstep, nb1, false);
        if ((unsigned)up < (unsigned)nb1) {
            const int vp = pdf_bin(y, pv[2 * up], pv[2 * up + 1], nb2, false);
            if ((unsigned)vp < (unsigned)nb2) atomicAdd(&tab[(vp * nb1 + up) * rep + rl], 1u);
        }
        if (vol) {
            const int uv = pdf_bin(x, vmin, vstep, nb1, false);
            if ((unsigned)uv < (unsigned)nb1) {
                const int vp = pdf_bin(y, vv[2 * uv], vv[2 * uv + 1], nb2, false);
                if ((unsigned)vp < (unsigned)nb2) atomicAdd(&tab[nw + (vp * nb1 + uv) * rep + rl], 1u);
            }
        }
    });
    __syncthreads();
    unsigned *out = a.cnt + ((size_t)c * a.ny + j) * a.ntab * nb;
    for (int t = threadIdx.x; t < a.ntab * nb; t += PDF_THREADS) {
        unsigned s = 0u;
        for (int r = 0; r < rep; ++r) s += tab[t * rep + ((r + threadIdx.x) & (rep - 1))];
        out[t] = s;
    }
}

__global__ void __launch_bounds__(PDF_THREADS) k_gate_threshold(const double *__restrict__ a, long long n, double thr, signed char *__restrict__ gate) {
    const long long stride = (long long)gridDim.x * PDF_THREADS;
    for (long long i = (long long)blockIdx.x * PDF_THREADS + threadIdx.x; i < n; i += stride) gate[i] = a[i] > thr ? 1 : 0;
}

// ---- INTER1V2D (utils/averages.f90:214-239) for every plane and level at once: the counts of gate == 1 .. np -------------------------------------
// k_gate_count: the grid and the rows of k_pdf_hist, grid (ny, nchunks).  A row is nx gate bytes; where its first byte is 16-byte aligned (the same
// for every lane of the wave) a lane takes 16 of them per load and the rest of the row goes byte by byte, otherwise the whole row does.  Level g in
// 1 .. np adds to tab[(g - 1) GATE_REP + lane % GATE_REP], a 32-bit counter in LDS; every other value, 0 included, is not counted.  The counts of
// the workgroup go to cnt[c][j][np] with plain vector stores.
constexpr int GATE_REP = 32;

__global__ void __launch_bounds__(PDF_THREADS) k_gate_count(const signed char *__restrict__ gate, int nx, int ny, int nz, int np,
                                                            unsigned *__restrict__ cnt) {
    __shared__ unsigned tab[GATE_MAX_LEVELS * GATE_REP];      // [np][GATE_REP]
    const int j = blockIdx.x, c = blockIdx.y, wave = threadIdx.x >> 6, lane = threadIdx.x & 63, rl = lane & (GATE_REP - 1);
    for (int t = threadIdx.x; t < np * GATE_REP; t += PDF_THREADS) tab[t] = 0u;
    __syncthreads();
    auto count = [&](int g) {
        if (g >= 1 && g <= np) atomicAdd(&tab[(g - 1) * GATE_REP + rl], 1u);
    };
    const int k1 = min(nz, (c + 1) * PDF_ROWS_PER_GROUP);
    for (int k = c * PDF_ROWS_PER_GROUP + wave; k < k1; k += PDF_WAVES) {
        const signed char *row = gate + ((size_t)k * ny + j) * nx;
        const int nvec = ((uintptr_t)row & 15) == 0 ? nx / 16 : 0;
        for (int i = lane; i < nvec; i += 64) {
            const uint4 v = reinterpret_cast<const uint4 *>(row)[i];
            const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int e = 0; e < 16; ++e) count((int)(signed char)(w[e >> 2] >> (8 * (e & 3))));
        }
        for (int i = nvec * 16 + lane; i < nx; i += 64) count((int)row[i]);
    }
    __syncthreads();
    unsigned *out = cnt + ((size_t)c * ny + j) * np;
    for (int t = threadIdx.x; t < np; t += PDF_THREADS) {
        unsigned s = 0u;
        for (int r = 0; r < GATE_REP; ++r) s += tab[t * GATE_REP + ((r + threadIdx.x) & (GATE_REP - 1))];      // (rotated, as in k_pdf_hist)
        out[t] = s;
    }
}

// inter[ip][j] = (the chunks of plane j, level ip + 1, as a 64-bit integer) / denom: grid (ny); one division per output, in fp64
__global__ void __launch_bounds__(PDF_THREADS) k_gate_count_final(const unsigned *__restrict__ cnt, int nchunks, int ny, int np, double denom,
                                                                  double *__restrict__ inter) {
    const int j = blockIdx.x;
    for (int ip = threadIdx.x; ip < np; ip += PDF_THREADS) {
        unsigned long long s = 0ull;
        for (int c = 0; c < nchunks; ++c) s += cnt[((size_t)c * ny + j) * np + ip];
        inter[(size_t)ip * ny + j] = (double)s / denom;
    }
}

bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

// the argument block of one launch; false: bad arguments
bool pdf_args(const PdfFields &F, PdfArgs &a, bool &vec) {
    if (F.nx < 1 || F.ny < 1 || F.nz < 1 || F.nv < 1 || F.nv > PDF_FIELDS_PER_LAUNCH || (F.igate != 0 && !F.gate)) return false;
    if (pdf_chunks(F.nz) > 65535) return false;
    vec = F.nx % 2 == 0;
    for (int i = 0; i < F.nv; ++i) {
        if (!F.f[i]) return false;
        a.f[i] = F.f[i];
        vec = vec && aligned16(F.f[i]);
    }
    a.gate = F.igate != 0 ? F.gate : nullptr; a.igate = F.igate; a.nx = F.nx; a.ny = F.ny; a.nz = F.nz;
    return true;
}

double pdf_bytes(const PdfFields &F) { return (double)F.nx * F.ny * (double)F.nz * (8.0 * F.nv + (F.igate != 0 ? 1.0 : 0.0)); }

}  // namespace

int pdf_chunks(int nz) { return (nz + PDF_ROWS_PER_GROUP - 1) / PDF_ROWS_PER_GROUP; }

int pdf_replicas(int nbins) {
    int rep = 32;
    while (rep > 1 && 2 * nbins * rep > PDF_LDS_WORDS) rep >>= 1;
    return rep;
}

hipError_t launch_pdf_minmax(const PdfFields &F, double *partial, double *mm, hipStream_t st) {
    PdfArgs a{};
    bool vec = false;
    if (!pdf_args(F, a, vec) || !partial || !mm) return hipErrorInvalidValue;
    a.partial = partial;
    const int nchunks = pdf_chunks(F.nz);
    const dim3 grid((unsigned)F.ny, (unsigned)nchunks, (unsigned)F.nv), block(PDF_THREADS);
    {
        ProfScope ps("k_pdf_minmax", st, pdf_bytes(F));
        if (a.gate) {
            if (vec) hipLaunchKernelGGL((k_pdf_minmax<2, true>), grid, block, 0, st, a);
            else hipLaunchKernelGGL((k_pdf_minmax<1, true>), grid, block, 0, st, a);
        } else {
            if (vec) hipLaunchKernelGGL((k_pdf_minmax<2, false>), grid, block, 0, st, a);
            else hipLaunchKernelGGL((k_pdf_minmax<1, false>), grid, block, 0, st, a);
        }
    }
    hipLaunchKernelGGL(k_pdf_minmax_final, dim3((unsigned)F.nv), block, 0, st, partial, nchunks, F.ny, mm);
    return hipGetLastError();
}

hipError_t launch_pdf_hist(const PdfFields &F, int nbins, unsigned ext_mask, unsigned vol_mask, const double *iv, unsigned *cnt,
                           unsigned long long *volpart, double *pdf, hipStream_t st) {
    PdfArgs a{};
    bool vec = false;
    if (!pdf_args(F, a, vec) || nbins < 1 || nbins > PDF_MAX_BINS || !iv || !cnt || !volpart || !pdf) return hipErrorInvalidValue;
    if (F.ny == 1) vol_mask = 0u;      // no volume plane
    a.iv = iv; a.cnt = cnt; a.nbins = nbins; a.rep = pdf_replicas(nbins); a.ntab = vol_mask ? 2 : 1; a.ext_mask = ext_mask; a.vol_mask = vol_mask;
    if (a.ntab * nbins * a.rep > PDF_LDS_WORDS) return hipErrorInvalidValue;
    const int nchunks = pdf_chunks(F.nz);
    const dim3 grid((unsigned)F.ny, (unsigned)nchunks, (unsigned)F.nv), block(PDF_THREADS);
    {
        ProfScope ps("k_pdf_hist", st, pdf_bytes(F));
        if (a.gate) {
            if (vec) hipLaunchKernelGGL((k_pdf_hist<2, true>), grid, block, 0, st, a);
            else hipLaunchKernelGGL((k_pdf_hist<1, true>), grid, block, 0, st, a);
        } else {
            if (vec) hipLaunchKernelGGL((k_pdf_hist<2, false>), grid, block, 0, st, a);
            else hipLaunchKernelGGL((k_pdf_hist<1, false>), grid, block, 0, st, a);
        }
    }
    hipLaunchKernelGGL(k_pdf_hist_planes, dim3((unsigned)F.ny, (unsigned)F.nv), block, 0, st, cnt, nchunks, F.ny, a.ntab, nbins, vol_mask, pdf, volpart);
    if (F.ny > 1)
        hipLaunchKernelGGL(k_pdf_hist_volume, dim3((unsigned)((nbins + 63) / 64), (unsigned)F.nv), block, 0, st, volpart, F.ny, nbins, pdf);
    return hipGetLastError();
}

hipError_t launch_pdf2v_range(const PdfFields &F, int nb1, const double *iv, double *partial, double *volpart, double *rng, hipStream_t st) {
    PdfArgs a{};
    bool vec = false;
    if (!pdf_args(F, a, vec) || F.nv != 2 || F.igate != 0 || nb1 < 1 || 2 * nb1 * 2 > PDF_LDS_WORDS / 2 || !iv || !partial || !volpart || !rng)
        return hipErrorInvalidValue;
    a.iv = iv; a.partial = partial; a.nbins = nb1; a.ntab = F.ny > 1 ? 2 : 1;
    const int nchunks = pdf_chunks(F.nz);
    const dim3 grid((unsigned)F.ny, (unsigned)nchunks), block(PDF_THREADS);
    {
        ProfScope ps("k_pdf2v_range", st, pdf_bytes(F));
        if (vec) hipLaunchKernelGGL((k_pdf2v_range<2>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((k_pdf2v_range<1>), grid, block, 0, st, a);
    }
    hipLaunchKernelGGL(k_pdf2v_range_planes, dim3((unsigned)F.ny), block, 0, st, partial, nchunks, F.ny, a.ntab, nb1, rng, volpart);
    if (F.ny > 1) hipLaunchKernelGGL(k_pdf2v_range_volume, dim3((unsigned)((2 * nb1 + 63) / 64)), block, 0, st, volpart, F.ny, nb1, rng);
    return hipGetLastError();
}

hipError_t launch_pdf2v_hist(const PdfFields &F, int nb1, int nb2, const double *iv, const double *viv, unsigned *cnt, unsigned long long *volpart,
                             double *pdf, hipStream_t st) {
    PdfArgs a{};
    bool vec = false;
    if (!pdf_args(F, a, vec) || F.nv != 2 || F.igate != 0 || nb1 < 1 || nb2 < 1 || (long long)nb1 * nb2 > PDF_MAX_BINS || !iv || !viv || !cnt ||
        !volpart || !pdf)
        return hipErrorInvalidValue;
    const int nb = nb1 * nb2;
    a.iv = iv; a.cnt = cnt; a.nbins = nb; a.rep = pdf_replicas(nb); a.ntab = F.ny > 1 ? 2 : 1;
    if (a.ntab * nb * a.rep > PDF_LDS_WORDS) return hipErrorInvalidValue;
    const int nchunks = pdf_chunks(F.nz);
    const dim3 grid((unsigned)F.ny, (unsigned)nchunks), block(PDF_THREADS);
    {
        ProfScope ps("k_pdf2v_hist", st, pdf_bytes(F));
        if (vec) hipLaunchKernelGGL((k_pdf2v_hist<2>), grid, block, 0, st, a, viv, nb1, nb2);
        else hipLaunchKernelGGL((k_pdf2v_hist<1>), grid, block, 0, st, a, viv, nb1, nb2);
    }
    hipLaunchKernelGGL(k_pdf_hist_planes, dim3((unsigned)F.ny, 1u), block, 0, st, cnt, nchunks, F.ny, a.ntab, nb, a.ntab == 2 ? 1u : 0u, pdf, volpart);
    if (F.ny > 1) hipLaunchKernelGGL(k_pdf_hist_volume, dim3((unsigned)((nb + 63) / 64), 1u), block, 0, st, volpart, F.ny, nb, pdf);
    return hipGetLastError();
}

hipError_t launch_gate_count(const signed char *gate, int nx, int ny, int nz, int np, unsigned *cnt, double *inter, hipStream_t st) {
    if (!gate || !cnt || !inter || nx < 1 || ny < 1 || nz < 1 || np < 1 || np > GATE_MAX_LEVELS || pdf_chunks(nz) > 65535) return hipErrorInvalidValue;
    const int nchunks = pdf_chunks(nz);
    {
        ProfScope ps("k_gate_count", st, (double)nx * ny * (double)nz);
        hipLaunchKernelGGL(k_gate_count, dim3((unsigned)ny, (unsigned)nchunks), dim3(PDF_THREADS), 0, st, gate, nx, ny, nz, np, cnt);
    }
    hipLaunchKernelGGL(k_gate_count_final, dim3((unsigned)ny), dim3(PDF_THREADS), 0, st, cnt, nchunks, ny, np, (double)((long long)nx * nz), inter);
    return hipGetLastError();
}

hipError_t launch_gate_threshold(const double *a, long long n, double thr, signed char *gate, hipStream_t st) {
    if (!a || !gate || n < 1) return hipErrorInvalidValue;
    const long long nblocks = std::min<long long>((n + PDF_THREADS - 1) / PDF_THREADS, 65536);
    ProfScope ps("k_gate_threshold", st, 9.0 * (double)n);
    hipLaunchKernelGGL(k_gate_threshold, dim3((unsigned)nblocks), dim3(PDF_THREADS), 0, st, a, n, thr, gate);
    return hipGetLastError();
}

}  // namespace tlab

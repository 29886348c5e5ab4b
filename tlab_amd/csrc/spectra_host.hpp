// Spectra and correlations in horizontal planes (spectra.hip, spectra.cpp): the index maps of module SpectraMod (tools/statistics/spectra_pool.f90)
// and of the kz shuffle of OPR_Fourier_Z_Forward (operators/opr_fourier.f90:357-370), written once for the kernels and for the host loops, and the
// ring lists of the radial sums.  Indices are 0-based here unless a name ends in 1.
//
// Layouts.  A transformed field is complex (nx/2+1, ny, nz), kx fastest, kz in the NATURAL order of the FFT (kz = 0, 1, .., nz/2, -(nz/2-1), .., -1).
// The reference shuffles kz before it reduces (fft_reordering_k): position ks of its arrays holds the natural mode spec_natural(ks).  The 2-D
// power out2d(nx/2, ny/nblock, nz) keeps the reference's shuffled order; the shuffle itself is never carried out as a pass.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

namespace tlab {

// The natural kz that the shuffle leaves at position ks: p_org(:, k) = p_dst(:, k + nz/2), p_org(:, k + nz/2) = p_dst(:, k) for k = 1 .. nz/2
// (opr_fourier.f90:358-366).  With odd nz the reference's loop does not reach the last position; it stays where it is here (the reference leaves
// the untransformed input there).
__host__ __device__ __forceinline__ int spec_natural(int ks, int nz) {
    const int h = nz / 2;
    return ks < h ? ks + h : (ks < 2 * h ? ks - h : ks);
}
__host__ __device__ __forceinline__ int spec_shifted(int kn, int nz) {      // the inverse map
    const int h = nz / 2;
    return kn < h ? kn + h : (kn < 2 * h ? kn - h : kn);
}

// INTEGRATE_SPECTRUM's view of position ks (spectra_pool.f90:84-88): kzg1 = kz_global (1-based, 1 the mean mode; the Nyquist mode nz/2+1 folded
// onto nz/2), flag = 1 for the first half of the positions (the negative kz, whose kx = 0 column is not counted)
struct SpecFold { int kzg1, flag; };
__host__ __device__ __forceinline__ SpecFold spec_fold(int ks, int nz) {
    const int h = nz / 2, k1 = ks + 1;
    SpecFold f;
    if (k1 <= h) { f.kzg1 = h - k1 + 2; f.flag = 1; }
    else { f.kzg1 = k1 - h; f.flag = 0; }
    if (f.kzg1 == h + 1) f.kzg1 = h > 1 ? h : 1;
    return f;
}

// int(sqrt(real(a**2 + b**2, wp))) of spectra_pool.f90:99, :349, :394: the 0-based ring.  sqrt is correctly rounded and a*a + b*b is exact, so a
// perfect square gives its root.  Host only: the kernels read the rings from the lists below.
inline int spec_ring(int a, int b) { return (int)std::sqrt((double)((long long)a * a + (long long)b * b)); }

// The modes of every ring in the reference's traversal order (position outer, kx inner): ring r holds mode[off[r]] .. mode[off[r + 1] - 1].
struct RingList {
    std::vector<int> off, mode;
};
// INTEGRATE_SPECTRUM (:75-117) on S(nkx, ., nz): mode = kx + nkx * ks.  The kx = 0 modes of the first half are added and taken away again there
// (:100-109): they are not listed.
inline RingList spectrum_rings(int nkx, int nz, int kr_total) {
    RingList L;
    std::vector<int> cnt(kr_total + 1, 0);
    for (int pass = 0; pass < 2; ++pass) {
        if (pass == 1) {
            L.off.assign(kr_total + 1, 0);
            for (int r = 0; r < kr_total; ++r) L.off[r + 1] = L.off[r] + cnt[r];
            L.mode.resize(L.off[kr_total]);
            std::fill(cnt.begin(), cnt.end(), 0);
        }
        for (int ks = 0; ks < nz; ++ks) {
            const SpecFold f = spec_fold(ks, nz);
            for (int i = 0; i < nkx; ++i) {
                const int r = spec_ring(i, f.kzg1 - 1);
                if (r >= kr_total || (i == 0 && f.flag == 1)) continue;
                if (pass == 1) L.mode[L.off[r] + cnt[r]] = i + nkx * ks;
                ++cnt[r];
            }
        }
    }
    return L;
}
// REDUCE_CORRELATION (:326-352) on in(nx, ., nz): mode = i + nx * k, no wrap-around of the separations
inline RingList correlation_rings(int nx, int nz, int nr_total) {
    RingList L;
    std::vector<int> cnt(nr_total + 1, 0);
    for (int pass = 0; pass < 2; ++pass) {
        if (pass == 1) {
            L.off.assign(nr_total + 1, 0);
            for (int r = 0; r < nr_total; ++r) L.off[r + 1] = L.off[r] + cnt[r];
            L.mode.resize(L.off[nr_total]);
            std::fill(cnt.begin(), cnt.end(), 0);
        }
        for (int k = 0; k < nz && k < nr_total; ++k)
            for (int i = 0; i < nx && i < nr_total; ++i) {
                const int r = spec_ring(k, i);
                if (r >= nr_total) continue;
                if (pass == 1) L.mode[L.off[r] + cnt[r]] = i + nx * k;
                ++cnt[r];
            }
    }
    return L;
}

}  // namespace tlab

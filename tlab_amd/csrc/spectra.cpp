// C ABI of the plane spectra and correlations (include/tlab_amd.h): tlab_spectrum_reduce (REDUCE_SPECTRUM + INTEGRATE_SPECTRUM of module SpectraMod,
// tools/statistics/spectra_pool.f90, fed with the transformed fields themselves), tlab_correlation_reduce (REDUCE_CORRELATION), tlab_radial_samplesize,
// tlab_cross_product, tlab_fluctuation, and the composed operators tlab_spectra_pair (the loop body of tools/statistics/spectra.f90:620-671 for one pair,
// on a Poisson plan's transforms) and tlab_dns_spectra (its pair list, :482-522, on the driver's arrays).  Device arrays take the kernels of
// spectra.hip, host arrays the reference's loops below; a host array never reaches a kernel, a device array is never read by the host.  The
// index maps are those of spectra_host.hpp on both sides.  Profiles (ny values) are host memory, as in averages.cpp.  From stats_common.hpp:
// on_device and Scratch.
#include "../../include/tlab_amd.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <memory>
#include <string>
#include <vector>

#include "driver_common.hpp"
#include "kernels.hpp"
#include "spectra_host.hpp"
#include "stats_common.hpp"

#pragma clang fp contract(off)      // every operation below stays as written

using namespace tlab;

namespace {

Scratch g_scratch("hipMalloc(spectra)");      // the device scratch of one call

// the ring lists of one (kind, line length, nz, number of rings) on the device; the last few are kept
// (like the scratch they are the process's: nothing is freed at exit, when the runtime may be gone; a list that leaves the cache is freed then)
struct DevRings {
    int kind, n1, nz, nr;
    int *off = nullptr, *mode = nullptr;
};
std::vector<std::unique_ptr<DevRings>> g_rings;
const DevRings &rings(int kind, int n1, int nz, int nr) {
    for (const auto &r : g_rings)
        if (r->kind == kind && r->n1 == n1 && r->nz == nz && r->nr == nr) return *r;
    const RingList L = kind == 0 ? spectrum_rings(n1, nz, nr) : correlation_rings(n1, nz, nr);
    auto r = std::make_unique<DevRings>();
    r->kind = kind; r->n1 = n1; r->nz = nz; r->nr = nr;
    hk(hipMalloc((void **)&r->off, L.off.size() * sizeof(int)), "hipMalloc(rings)");
    hk(hipMalloc((void **)&r->mode, std::max<size_t>(L.mode.size(), 1) * sizeof(int)), "hipMalloc(rings)");
    hk(hipMemcpy(r->off, L.off.data(), L.off.size() * sizeof(int), hipMemcpyHostToDevice), "hipMemcpy(rings)");
    if (!L.mode.empty()) hk(hipMemcpy(r->mode, L.mode.data(), L.mode.size() * sizeof(int), hipMemcpyHostToDevice), "hipMemcpy(rings)");
    if (g_rings.size() >= 8) {
        (void)hipFree(g_rings.front()->off);
        (void)hipFree(g_rings.front()->mode);
        g_rings.erase(g_rings.begin());
    }
    g_rings.push_back(std::move(r));
    return *g_rings.back();
}

void check_spectra_box(const std::string &who, int nx, int ny, int nz, int nblock) {
    if (nx < 2 || ny < 1 || nz < 1) throw Fail(TLAB_EINVAL, who + ": nx must be at least 2, ny and nz at least 1");
    if (nx % 2) throw Fail(TLAB_EINVAL, who + ": nx must be even");
    if (nblock < 1 || nblock > ny) throw Fail(TLAB_EINVAL, who + ": nblock must be 1 to ny");
    if (nz == 1) throw Fail(TLAB_EUNSUPPORTED, who + ": nz = 1 (no z transform) is not built");
    if ((long long)nx * nz > 0x7fffffffLL) throw Fail(TLAB_EINVAL, who + ": nx * nz does not fit the mode lists");
}

// ---- the reference's loops (host arrays) ---------------------------------------------------------------------------------------------------------
// REDUCE_SPECTRUM (spectra_pool.f90:232-274) on the product it is handed by OPR_Fourier_CONVOLUTION_FXZ (opr_fourier.f90:554, :563) and
// spectra.f90:641, then INTEGRATE_SPECTRUM (:73-185) and spectra.f90:669
void host_spectrum(int nx, int ny, int nz, int nblock, int kr_total, const double *a, const double *b, double *out2d, double *outx, double *outz,
                   double *outr, double *variance) {
    const int nkx = nx / 2, nxh = nkx + 1, nyo = ny / nblock, ny_loc = nyo * nblock, nkz = nz / 2;
    const double norm = 1.0 / (double)((long long)nx * nz);
    std::vector<double> S((size_t)nkx * nyo * nz, 0.0);
    std::fill(variance, variance + ny, 0.0);
    auto power = [&](size_t ip) {
        const double ar = a[2 * ip], ai = a[2 * ip + 1], br = b ? b[2 * ip] : ar, bi = b ? b[2 * ip + 1] : ai;
        const double p = br * ar + bi * ai;
        return (p * norm) * norm;
    };
    for (int ks = 0; ks < nz; ++ks) {
        const int kn = spec_natural(ks, nz);
        for (int y = 0; y < ny_loc; ++y) {
            const int jb = y / nblock;
            const size_t base = ((size_t)kn * ny + y) * nxh;
            for (int kx = 0; kx < nkx; ++kx) {
                const double p = power(base + kx);
                double &o = S[((size_t)ks * nyo + jb) * nkx + kx];
                o = o + p;
                if (kx == 0) variance[y] = variance[y] + p;
                else variance[y] = variance[y] + p * 2.0;
            }
            variance[y] = variance[y] + power(base + nkx);
        }
    }
    std::vector<double> tmp_x((size_t)nkx * nyo, 0.0), tmp_z((size_t)nyo * nz, 0.0), wrk((size_t)nyo * nz, 0.0);
    for (int ks = 0; ks < nz; ++ks) {
        const SpecFold f = spec_fold(ks, nz);
        const double *Sk = S.data() + (size_t)ks * nyo * nkx;
        for (size_t t = 0; t < (size_t)nkx * nyo; ++t) tmp_x[t] = tmp_x[t] + Sk[t];
        for (int i = 0; i < nkx; ++i) {
            const int kr = spec_ring(i, f.kzg1 - 1);
            for (int y = 0; y < nyo; ++y) {
                const double p = Sk[(size_t)y * nkx + i];
                double &tz = tmp_z[(size_t)ks * nyo + y];
                tz = tz + p;
                if (kr < kr_total) outr[(size_t)y * kr_total + kr] = outr[(size_t)y * kr_total + kr] + p;
                if (i == 0 && f.flag == 1) {
                    tz = tz - p;
                    if (kr < kr_total) outr[(size_t)y * kr_total + kr] = outr[(size_t)y * kr_total + kr] - p;
                }
                if (f.kzg1 == 1 && i > 0) tz = tz + p;
            }
        }
    }
    for (size_t t = 0; t < (size_t)nkx * nyo; ++t) outx[t] = outx[t] + tmp_x[t];
    for (int ks = 0; ks < nz; ++ks) {
        const int kzf = spec_fold(ks, nz).kzg1 - 1;
        for (int y = 0; y < nyo; ++y) wrk[(size_t)kzf * nyo + y] = wrk[(size_t)kzf * nyo + y] + tmp_z[(size_t)ks * nyo + y];
    }
    for (int k = 0; k < nkz; ++k)
        for (int y = 0; y < nyo; ++y) outz[(size_t)y * nkz + k] = outz[(size_t)y * nkz + k] + wrk[(size_t)k * nyo + y];
    if (out2d)
        for (size_t t = 0; t < S.size(); ++t) out2d[t] = out2d[t] + S[t];
}

// 1/(sqrt(var1) sqrt(var2)), or 1 where the product is not positive (spectra_pool.f90:321-324)
void corr_norms(int ny, const double *var1, const double *var2, double *normj) {
    for (int j = 0; j < ny; ++j) {
        const double n = std::sqrt(var1[j]) * std::sqrt(var2[j]);
        normj[j] = n > 0.0 ? 1.0 / n : 1.0;
    }
}

// spectra.f90:653, then REDUCE_CORRELATION (spectra_pool.f90:313-358); out2d: the tool's wrk3d, accumulated into as its out2d is (:669)
void host_correlation(int nx, int ny, int nz, int nblock, int nr_total, const double *in, const double *normj, double *out2d, double *outx,
                      double *outz, double *outr, double *variance2) {
    const int nyo = ny / nblock, ny_loc = nyo * nblock;
    const double norm = 1.0 / (double)((long long)nx * nz);
    std::fill(variance2, variance2 + ny, 0.0);
    for (int j = 0; j < ny_loc; ++j) {
        const int jb = j / nblock;
        for (int k = 0; k < nz; ++k)
            for (int i = 0; i < nx; ++i) {
                const double x = (in[((size_t)k * ny + j) * nx + i] * norm) * norm, v = x * normj[j];
                if (out2d) out2d[((size_t)k * nyo + jb) * nx + i] = out2d[((size_t)k * nyo + jb) * nx + i] + v;
                if (k == 0) outx[(size_t)jb * nx + i] = outx[(size_t)jb * nx + i] + v;
                if (i == 0) outz[(size_t)jb * nz + k] = outz[(size_t)jb * nz + k] + v;
                if (outr) {
                    const int r = spec_ring(k, i);
                    if (r < nr_total) outr[(size_t)jb * nr_total + r] = outr[(size_t)jb * nr_total + r] + v;
                }
                if (i == 0 && k == 0) variance2[j] = x;
            }
    }
}

// ---- the two reductions on arrays of either kind ---------------------------------------------------------------------------------------------------
void spectrum_reduce(const char *who, bool dev, int nx, int ny, int nz, int nblock, int kr_total, const double *a, const double *b, double *out2d,
                     double *outx, double *outz, double *outr, double *variance) {
    if (!dev) {
        host_spectrum(nx, ny, nz, nblock, kr_total, a, b, out2d, outx, outz, outr, variance);
        return;
    }
    hipStream_t st = tlab_current_stream();
    const int nkx = nx / 2, nyo = ny / nblock;
    const size_t nS = (size_t)nkx * nyo * nz, nrow = (size_t)ny * nz;
    const DevRings &R = rings(0, nkx, nz, kr_total);
    double *S = g_scratch.doubles(nS + nrow + ny), *rowv = S + nS, *dvar = rowv + nrow;
    hk(launch_spectrum_reduce(nx, ny, nz, nblock, kr_total, a, b, S, rowv, R.off, R.mode, out2d, outx, outz, outr, dvar, st), who);
    hk(hipMemcpyAsync(variance, dvar, (size_t)ny * sizeof(double), hipMemcpyDeviceToHost, st), "hipMemcpy(variance)");
    hk(hipStreamSynchronize(st), "sync");
}

void correlation_reduce(const char *who, bool dev, int nx, int ny, int nz, int nblock, int nr_total, const double *in, const double *var1,
                        const double *var2, double *out2d, double *outx, double *outz, double *outr, double *variance2) {
    std::vector<double> normj(ny);
    corr_norms(ny, var1, var2, normj.data());
    if (!dev) {
        host_correlation(nx, ny, nz, nblock, nr_total, in, normj.data(), out2d, outx, outz, outr, variance2);
        return;
    }
    hipStream_t st = tlab_current_stream();
    const DevRings *R = outr ? &rings(1, nx, nz, nr_total) : nullptr;
    double *dnorm = g_scratch.doubles(2 * (size_t)ny), *dvar = dnorm + ny;
    hk(hipMemcpyAsync(dnorm, normj.data(), (size_t)ny * sizeof(double), hipMemcpyHostToDevice, st), "hipMemcpy(norms)");
    hk(launch_correlation_reduce(nx, ny, nz, nblock, nr_total, in, dnorm, R ? R->off : nullptr, R ? R->mode : nullptr, out2d, outx, outz, outr, dvar, st),
       who);
    hk(hipMemcpyAsync(variance2, dvar, (size_t)ny * sizeof(double), hipMemcpyDeviceToHost, st), "hipMemcpy(variance2)");
    hk(hipStreamSynchronize(st), "sync");      // (normj lives until here)
}

// spectra.f90:620-659 for one pair of fluctuation fields on the device; tmp: three arrays of (nx + 2) * ny * nz doubles
void spectra_pair(const char *who, tlab_poisson_plan_t plan, int nx, int ny, int nz, int mode, int nblock, int kr_total, const double *a,
                  const double *b, double *const *tmp, double *out2d, double *outx, double *outz, double *outr, double *cov, double *variance) {
    hipStream_t st = tlab_current_stream();
    ok(tlab_avg_cov2v(nx, ny, nz, a, b ? b : a, cov, ny), "tlab_avg_cov2v");      // wrk1d(:, 1:3), :624-628
    double *ah = tmp[1], *bh = b ? tmp[2] : nullptr;
    ok(tlab_poisson_fft_x(plan, +1, const_cast<double *>(a), tmp[0]), "tlab_poisson_fft_x");
    ok(tlab_poisson_fft_z(plan, +1, tmp[0], ah), "tlab_poisson_fft_z");
    if (b) {
        ok(tlab_poisson_fft_x(plan, +1, const_cast<double *>(b), tmp[0]), "tlab_poisson_fft_x");
        ok(tlab_poisson_fft_z(plan, +1, tmp[0], bh), "tlab_poisson_fft_z");
    }
    if (mode == 1) {
        spectrum_reduce(who, true, nx, ny, nz, nblock, kr_total, ah, bh, out2d, outx, outz, outr, variance);
        return;
    }
    double *c = b ? bh : ah;
    hk(launch_cross_product(ah, bh, c, (long long)(nx / 2 + 1) * ny * nz, st), "k_cross_product");
    ok(tlab_poisson_fft_z(plan, -1, c, tmp[0]), "tlab_poisson_fft_z");
    ok(tlab_poisson_fft_x(plan, -1, tmp[0], tmp[1]), "tlab_poisson_fft_x");
    correlation_reduce(who, true, nx, ny, nz, nblock, kr_total, tmp[1], cov + ny, cov + 2 * (size_t)ny, out2d, outx, outz, outr, variance);
}

void check_pair(const std::string &who, int mode, const std::vector<const void *> &arrays) {
    if (mode != 1 && mode != 2) throw Fail(TLAB_EINVAL, who + ": mode must be 1 (spectra) or 2 (correlations)");
    for (const void *p : arrays)
        if (!p) throw Fail(TLAB_EINVAL, who + ": a null pointer");
    if (!on_device(who.c_str(), arrays)) throw Fail(TLAB_EINVAL, who + ": the arrays must be device memory");
}

}  // namespace

extern "C" {

int tlab_spectrum_reduce(int nx, int ny, int nz, int nblock, int kr_total, const double *a_hat, const double *b_hat, double *out2d, double *outx,
                         double *outz, double *outr, double *variance) {
    (void)tlab_internal_deferred_flush();
    return catch_fail([&] {
        const char *who = "tlab_spectrum_reduce";
        check_spectra_box(who, nx, ny, nz, nblock);
        if (kr_total < 1) throw Fail(TLAB_EINVAL, std::string(who) + ": kr_total must be at least 1");
        if (!a_hat || !outx || !outz || !outr || !variance) throw Fail(TLAB_EINVAL, std::string(who) + ": a null pointer");
        std::vector<const void *> all{a_hat, outx, outz, outr};
        if (b_hat) all.push_back(b_hat);
        if (out2d) all.push_back(out2d);
        spectrum_reduce(who, on_device(who, all), nx, ny, nz, nblock, kr_total, a_hat, b_hat, out2d, outx, outz, outr, variance);
    }, TLAB_EINVAL);
}

int tlab_correlation_reduce(int nx, int ny, int nz, int nblock, int nr_total, const double *in, const double *var1, const double *var2, double *out2d,
                            double *outx, double *outz, double *outr, double *variance2, int icalc_radial) {
    (void)tlab_internal_deferred_flush();
    return catch_fail([&] {
        const char *who = "tlab_correlation_reduce";
        check_spectra_box(who, nx, ny, nz, nblock);
        if (!in || !var1 || !var2 || !outx || !outz || !variance2) throw Fail(TLAB_EINVAL, std::string(who) + ": a null pointer");
        if (icalc_radial == 1 && (!outr || nr_total < 1)) throw Fail(TLAB_EINVAL, std::string(who) + ": icalc_radial = 1 needs outr and nr_total >= 1");
        double *r = icalc_radial == 1 ? outr : nullptr;
        std::vector<const void *> all{in, outx, outz};
        if (r) all.push_back(r);
        if (out2d) all.push_back(out2d);
        correlation_reduce(who, on_device(who, all), nx, ny, nz, nblock, nr_total, in, var1, var2, out2d, outx, outz, r, variance2);
    }, TLAB_EINVAL);
}

// RADIAL_SAMPLESIZE (spectra_pool.f90:381-398) from zero, as spectra.f90:674-675 calls it
int tlab_radial_samplesize(int nx, int nz, int nr_total, double *samplesize) {
    return catch_fail([&] {
        if (nx < 1 || nz < 1 || nr_total < 1 || !samplesize) throw Fail(TLAB_EINVAL, "tlab_radial_samplesize: nx, nz or nr_total < 1, or a null pointer");
        std::fill(samplesize, samplesize + nr_total, 0.0);
        for (int k = 0; k < nz; ++k)
            for (int i = 0; i < nx; ++i) {
                const int r = spec_ring(k, i);
                if (r < nr_total) samplesize[r] = samplesize[r] + 1.0;
            }
    }, TLAB_EINVAL);
}

int tlab_cross_product(long long n, const double *a_hat, const double *b_hat, double *c) {
    (void)tlab_internal_deferred_flush();
    return catch_fail([&] {
        const char *who = "tlab_cross_product";
        if (n < 1 || !a_hat || !c) throw Fail(TLAB_EINVAL, std::string(who) + ": n < 1 or a null pointer");
        std::vector<const void *> all{a_hat, c};
        if (b_hat) all.push_back(b_hat);
        if (on_device(who, all)) {
            hk(launch_cross_product(a_hat, b_hat, c, n, tlab_current_stream()), "k_cross_product");
            return;
        }
        for (long long i = 0; i < n; ++i) {
            const double ar = a_hat[2 * i], ai = a_hat[2 * i + 1], br = b_hat ? b_hat[2 * i] : ar, bi = b_hat ? b_hat[2 * i + 1] : ai;
            c[2 * i] = br * ar + bi * ai;
            c[2 * i + 1] = bi * ar - br * ai;
        }
    }, TLAB_EINVAL);
}

// FI_FLUCTUATION_INPLACE (mappings/fi_dissipation.f90:119-139) into another array, with the means handed in
int tlab_fluctuation(int nx, int ny, int nz, const double *in, const double *mean, double *out) {
    (void)tlab_internal_deferred_flush();
    return catch_fail([&] {
        const char *who = "tlab_fluctuation";
        if (nx < 1 || ny < 1 || nz < 1 || !in || !mean || !out) throw Fail(TLAB_EINVAL, std::string(who) + ": nx, ny or nz < 1, or a null pointer");
        if (!on_device(who, {in, out})) {
            for (int k = 0; k < nz; ++k)
                for (int j = 0; j < ny; ++j)
                    for (int i = 0; i < nx; ++i) out[((size_t)k * ny + j) * nx + i] = in[((size_t)k * ny + j) * nx + i] - mean[j];
            return;
        }
        hipStream_t st = tlab_current_stream();
        double *dm = g_scratch.doubles(ny);
        hk(hipMemcpyAsync(dm, mean, (size_t)ny * sizeof(double), hipMemcpyHostToDevice, st), "hipMemcpy(means)");
        hk(launch_fluctuation(nx, ny, nz, in, dm, out, st), "k_fluctuation");
        hk(hipStreamSynchronize(st), "sync");      // (the caller's means may go, and the scratch may be taken again)
    }, TLAB_EINVAL);
}

int tlab_spectra_pair(tlab_poisson_plan_t plan, int mode, int nblock, int kr_total, const double *a, const double *b, double *tmp1, double *tmp2,
                      double *tmp3, double *out2d, double *outx, double *outz, double *outr, double *cov, double *variance) {
    (void)tlab_internal_deferred_flush();
    return guarded([&] {
        const char *who = "tlab_spectra_pair";
        int n[3];
        if (!plan) throw Fail(TLAB_EINVAL, std::string(who) + ": null plan");
        if (!tlab_internal_poisson_box(plan, n)) throw Fail(TLAB_EUNSUPPORTED, std::string(who) + ": needs a single-device plan (no slab or pencil plan)");
        check_spectra_box(who, n[0], n[1], n[2], nblock);
        if (kr_total < 1) throw Fail(TLAB_EINVAL, std::string(who) + ": kr_total must be at least 1");
        if (!cov || !variance) throw Fail(TLAB_EINVAL, std::string(who) + ": a null pointer");
        std::vector<const void *> all{a, tmp1, tmp2, tmp3, outx, outz, outr};
        if (b) all.push_back(b);
        if (out2d) all.push_back(out2d);
        check_pair(who, mode, all);
        double *tmp[3] = {tmp1, tmp2, tmp3};
        if (tmp1 == tmp2 || tmp1 == tmp3 || tmp2 == tmp3) throw Fail(TLAB_EINVAL, std::string(who) + ": the work arrays must be distinct");
        spectra_pair(who, plan, n[0], n[1], n[2], mode, nblock, kr_total, a, b == a ? nullptr : b, tmp, out2d, outx, outz, outr, cov, variance);
    });
}

int tlab_dns_spectra(tlab_dns_t h, int mode, int cross, int nblock, int kr_total, double *const *q, double *const *s, double *const *txc,
                     const double *p, double *out2d, double *outx, double *outz, double *outr, double *cov, double *variance) {
    (void)tlab_internal_deferred_flush();
    return guarded([&] {
        const char *who = "tlab_dns_spectra";
        if (!h) throw Fail(TLAB_EINVAL, std::string(who) + ": null handle");
        tlab_dns_grid G;
        tlab_internal_dns_grid(h, &G);
        const int nx = G.nx, ny = G.ny, nz = G.nz, nscal = tlab_internal_dns_nscal(h);
        tlab_poisson_plan_t plan = tlab_internal_dns_poisson(h);
        check_spectra_box(who, nx, ny, nz, nblock);
        if (kr_total < 1) throw Fail(TLAB_EINVAL, std::string(who) + ": kr_total must be at least 1");
        if (!q || !txc || (nscal > 0 && !s) || !outx || !outz || !outr || !cov || !variance) throw Fail(TLAB_EINVAL, std::string(who) + ": a null pointer");
        std::vector<const double *> var{q[0], q[1], q[2]};      // vars(:), spectra.f90:454-474
        if (p) var.push_back(p);
        const int iv_offset = (int)var.size();
        for (int is = 0; is < nscal; ++is) var.push_back(s[is]);
        std::vector<const void *> all(var.begin(), var.end());
        static const int work[5] = {0, 1, 3, 4, 5};             // (txc[2] is where FI_PRESSURE_BOUSSINESQ leaves p)
        for (int i : work) {
            if (!txc[i]) throw Fail(TLAB_EINVAL, std::string(who) + ": a null work array");
            for (const double *v : var)
                if (v == txc[i]) throw Fail(TLAB_EINVAL, std::string(who) + ": a field is one of the work arrays txc[0, 1, 3, 4, 5]");
            all.push_back(txc[i]);
        }
        all.push_back(outx); all.push_back(outz); all.push_back(outr);
        if (out2d) all.push_back(out2d);
        check_pair(who, mode, all);
        std::vector<std::pair<int, int>> pairs;                 // p_pairs, :482-522
        if (!cross)
            for (int i = 0; i < (int)var.size(); ++i) pairs.push_back({i, i});
        else {
            pairs = {{0, 1}, {0, 2}, {1, 2}};
            for (int is = 0; is < nscal; ++is)
                for (int i = 0; i < 3; ++i) pairs.push_back({i, iv_offset + is});
        }
        const int nv = (int)var.size(), nyo = ny / nblock;
        std::vector<double> mean((size_t)nv * ny);
        for (int v0 = 0; v0 < nv; v0 += 8)
            ok(tlab_avg_ik_v(nx, ny, nz, std::min(8, nv - v0), var.data() + v0, mean.data() + (size_t)v0 * ny, ny), "tlab_avg_ik_v");
        const size_t n1 = mode == 1 ? nx / 2 : nx, nz1 = mode == 1 ? nz / 2 : nz;
        double *tmp[3] = {txc[3], txc[4], txc[5]};
        for (size_t ip = 0; ip < pairs.size(); ++ip) {
            const int i1 = pairs[ip].first, i2 = pairs[ip].second;
            ok(tlab_fluctuation(nx, ny, nz, var[i1], mean.data() + (size_t)i1 * ny, txc[0]), "tlab_fluctuation");
            if (i2 != i1) ok(tlab_fluctuation(nx, ny, nz, var[i2], mean.data() + (size_t)i2 * ny, txc[1]), "tlab_fluctuation");
            spectra_pair(who, plan, nx, ny, nz, mode, nblock, kr_total, txc[0], i2 != i1 ? txc[1] : nullptr, tmp,
                         out2d ? out2d + ip * n1 * nyo * nz : nullptr, outx + ip * n1 * nyo, outz + ip * nz1 * nyo, outr + ip * (size_t)kr_total * nyo,
                         cov + ip * 3 * (size_t)ny, variance + ip * (size_t)ny);
        }
    });
}

}  // extern "C"

// C ABI of the plane PDFs (include/tlab_amd.h): tlab_pdf1v_n (PDF1V_N, statistics/pdf.f90:14-91, without its file), its two passes on their own
// tlab_pdf_minmax_planes / tlab_pdf_histogram_planes, tlab_pdf_analize (PDF_ANALIZE, host arithmetic), tlab_pdf2v (PDF2V, :123-159) and
// tlab_gate_threshold, and the intermittency factors of a gate, tlab_inter_n_xz (INTER_N_XZ, statistics/avg_xz.f90:109-153).  Device arrays take the kernels of pdfs.hip, host arrays the reference's loops below; a host array never reaches a kernel, a
// device array is never read by the host.  The bin of a point, the step of an interval and PDF_ANALIZE are those of pdfs_host.hpp on both sides;
// every interval bound is computed HERE, on the host, for both kinds of array.
#include "../../include/tlab_amd.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "driver_common.hpp"
#include "kernels.hpp"
#include "pdfs_host.hpp"

#pragma clang fp contract(off)      // every operation below stays as written

using namespace tlab;

namespace {

// device scratch of one pass: one buffer for the process, grown on demand (the calls run on the library's stream one after the other)
char *g_buf = nullptr;
size_t g_buf_n = 0;
char *scratch(size_t bytes) {
    if (g_buf_n < bytes) {
        if (g_buf) hk(hipFree(g_buf), "hipFree");
        g_buf = nullptr; g_buf_n = 0;
        hk(hipMalloc((void **)&g_buf, bytes), "hipMalloc(plane PDFs)");
        g_buf_n = bytes;
    }
    return g_buf;
}
size_t up16(size_t n) { return (n + 15) & ~(size_t)15; }

struct Box {
    const char *who;
    bool dev;
    int nx, ny, nz, igate;
    const signed char *gate;
    size_t plane() const { return (size_t)nx * nz; }
};

// 1: every array is device memory, 0: every array is host memory (or no tlab_init: no array is the library's); a mix is refused
bool on_device(const char *who, const std::vector<const void *> &p) {
    size_t ndev = 0;
    if (tlab_device_ready())
        for (const void *x : p) {
            const int on = tlab_pointer_on_device(x);
            if (on < 0) throw Fail(on, std::string(who) + ": " + tlab_last_error());
            ndev += on ? 1 : 0;
        }
    if (ndev != 0 && ndev != p.size()) throw Fail(TLAB_EINVAL, std::string(who) + ": host and device arrays in one call");
    return ndev != 0;
}

Box check_box(const char *who, int nx, int ny, int nz, int nv, const double *const *u, int igate, const signed char *gate) {
    if (nx < 1 || ny < 1 || nz < 1) throw Fail(TLAB_EINVAL, std::string(who) + ": nx, ny, nz must be at least 1");
    if (nv < 1 || !u) throw Fail(TLAB_EINVAL, std::string(who) + ": nv < 1 or a null pointer");
    if (igate < -128 || igate > 127) throw Fail(TLAB_EINVAL, std::string(who) + ": igate is not a value of an int8 gate");
    if (igate != 0 && !gate) throw Fail(TLAB_EINVAL, std::string(who) + ": igate != 0 needs a gate");
    std::vector<const void *> all;
    for (int v = 0; v < nv; ++v) {
        if (!u[v]) throw Fail(TLAB_EINVAL, std::string(who) + ": a null field");
        all.push_back(u[v]);
    }
    if (igate != 0) all.push_back(gate);
    return Box{who, on_device(who, all), nx, ny, nz, igate, igate != 0 ? gate : nullptr};
}

void check_bins(const char *who, long long nbins) {
    if (nbins < 1 || nbins > PDF_MAX_BINS) throw Fail(TLAB_EINVAL, std::string(who) + ": the number of bins must be 1 to " + std::to_string(PDF_MAX_BINS));
}

// ---- the reference's loops (host arrays) ---------------------------------------------------------------------------------------------------------
// plane j of u(nx, ny, nz) is u(:, j, :); the volume is the same loop over u(nx*ny, 1, nz), that is every point (statistics/pdf.f90:74)
template <class F>
void for_plane(const Box &B, int j, F &&fn) {
    if (j < B.ny) {
        for (int k = 0; k < B.nz; ++k)
            for (int i = 0; i < B.nx; ++i) fn(((size_t)k * B.ny + j) * B.nx + i);
    } else {
        const size_t n = (size_t)B.nx * B.ny * B.nz;
        for (size_t i = 0; i < n; ++i) fn(i);
    }
}

// utils/pdfs.f90:50-57 (from the first point) and :144-153 (gated: from big_wp); mm: [ny + 1][2]
void host_minmax(const Box &B, const double *u, double *mm) {
    for (int j = 0; j <= B.ny; ++j) {
        double mn, mx;
        if (B.gate) { mn = PDF_BIG; mx = -PDF_BIG; }
        else mn = mx = u[j < B.ny ? (size_t)j * B.nx : 0];
        for_plane(B, j, [&](size_t i) {
            if (B.gate && B.gate[i] != B.igate) return;
            mn = u[i] < mn ? u[i] : mn;
            mx = u[i] > mx ? u[i] : mx;
        });
        mm[2 * j] = mn; mm[2 * j + 1] = mx;
    }
}

// :76-90, :172-189; iv: [ny + 1][2] = (umin, ustep); cnt: [ny + 1][nbins]
void host_hist(const Box &B, const double *u, int nbins, bool ext, const double *iv, double *cnt) {
    for (int j = 0; j < B.ny + (B.ny > 1 ? 1 : 0); ++j) {
        double *c = cnt + (size_t)j * nbins;
        const double umin = iv[2 * j], ustep = iv[2 * j + 1];
        for_plane(B, j, [&](size_t i) {
            if (B.gate && B.gate[i] != B.igate) return;
            const int b = pdf_bin(u[i], umin, ustep, nbins, ext);
            if (b >= 0 && b < nbins) c[b] += 1.0;
        });
    }
}

// ---- the passes ----------------------------------------------------------------------------------------------------------------------------------
PdfFields group(const Box &B, const double *const *u, const std::vector<int> &idx, size_t v0) {
    PdfFields F{};
    F.nv = (int)std::min<size_t>(PDF_FIELDS_PER_LAUNCH, idx.size() - v0);
    for (int i = 0; i < F.nv; ++i) F.f[i] = u[idx[v0 + i]];
    F.gate = B.gate; F.igate = B.igate; F.nx = B.nx; F.ny = B.ny; F.nz = B.nz;
    return F;
}

// min and max of the fields idx: mm [idx.size()][ny + 1][2], the volume as plane ny.  One synchronisation.
void minmax_pass(const Box &B, const double *const *u, const std::vector<int> &idx, std::vector<double> &mm) {
    const size_t ns = idx.size(), np = (size_t)B.ny + 1;
    mm.assign(ns * np * 2, 0.0);
    if (ns == 0) return;
    if (!B.dev) {
        for (size_t s = 0; s < ns; ++s) host_minmax(B, u[idx[s]], mm.data() + s * np * 2);
        return;
    }
    hipStream_t st = tlab_current_stream();
    const size_t npart = (size_t)PDF_FIELDS_PER_LAUNCH * pdf_chunks(B.nz) * B.ny * 2;
    double *dmm = (double *)scratch((ns * np * 2 + npart) * sizeof(double)), *partial = dmm + ns * np * 2;
    for (size_t v0 = 0; v0 < ns; v0 += PDF_FIELDS_PER_LAUNCH)
        hk(launch_pdf_minmax(group(B, u, idx, v0), partial, dmm + v0 * np * 2, st), "k_pdf_minmax");
    hk(hipMemcpyAsync(mm.data(), dmm, mm.size() * sizeof(double), hipMemcpyDeviceToHost, st), "hipMemcpy(min/max)");
    hk(hipStreamSynchronize(st), "sync");
}

// The histograms of the fields idx on the intervals lo, hi [idx.size()][ny + 1] (the volume's as plane ny), ext[s]: external (a point outside is
// dropped).  Writes the whole of pdf(nbins + 2, ny + 1) of field idx[s] at pdf + idx[s] * ldf: counts and the two centres; with ny == 1 the last
// plane is zero.  One synchronisation.
void hist_pass(const Box &B, const double *const *u, const std::vector<int> &idx, int nbins, const std::vector<char> &ext, const std::vector<double> &lo,
               const std::vector<double> &hi, double *pdf, size_t ldf) {
    const size_t ns = idx.size(), np = (size_t)B.ny + 1, npl = B.ny > 1 ? np : 1;
    if (ns == 0) return;
    std::vector<double> iv(ns * np * 2, 1.0), cnt(ns * np * nbins, 0.0);
    std::vector<char> vol(ns, 0);
    for (size_t s = 0; s < ns; ++s) {
        double *out = pdf + idx[s] * ldf;
        std::fill(out, out + np * (nbins + 2), 0.0);
        for (size_t j = 0; j < npl; ++j) {
            double *p = out + j * (nbins + 2);
            iv[(s * np + j) * 2] = lo[s * np + j];
            iv[(s * np + j) * 2 + 1] = pdf_step(lo[s * np + j], hi[s * np + j], nbins, p + nbins, p + nbins + 1);
        }
        // the volume is binned on its own unless every plane has its interval: then its counts are the sum of the planes'
        for (size_t j = 0; j < (size_t)B.ny && B.ny > 1; ++j)
            if (!(iv[(s * np + j) * 2] == iv[(s * np + B.ny) * 2] && iv[(s * np + j) * 2 + 1] == iv[(s * np + B.ny) * 2 + 1])) vol[s] = 1;
    }
    if (!B.dev) {
        for (size_t s = 0; s < ns; ++s) host_hist(B, u[idx[s]], nbins, ext[s] != 0, iv.data() + s * np * 2, cnt.data() + s * np * nbins);
    } else {
        hipStream_t st = tlab_current_stream();
        const size_t ncnt = (size_t)PDF_FIELDS_PER_LAUNCH * pdf_chunks(B.nz) * B.ny * 2 * nbins, nvp = (size_t)PDF_FIELDS_PER_LAUNCH * B.ny * nbins;
        const size_t o_pdf = up16(iv.size() * 8), o_vp = o_pdf + up16(cnt.size() * 8), o_cnt = o_vp + up16(nvp * 8);
        char *buf = scratch(o_cnt + up16(ncnt * 4));
        double *div = (double *)buf, *dpdf = (double *)(buf + o_pdf);
        hk(hipMemcpyAsync(div, iv.data(), iv.size() * sizeof(double), hipMemcpyHostToDevice, st), "hipMemcpy(intervals)");
        for (size_t v0 = 0; v0 < ns; v0 += PDF_FIELDS_PER_LAUNCH) {
            const PdfFields F = group(B, u, idx, v0);
            unsigned em = 0u, vm = 0u;
            for (int i = 0; i < F.nv; ++i) {
                em |= ext[v0 + i] ? 1u << i : 0u;
                vm |= vol[v0 + i] ? 1u << i : 0u;
            }
            hk(launch_pdf_hist(F, nbins, em, vm, div + v0 * np * 2, (unsigned *)(buf + o_cnt), (unsigned long long *)(buf + o_vp),
                               dpdf + v0 * np * nbins, st), "k_pdf_hist");
        }
        hk(hipMemcpyAsync(cnt.data(), dpdf, cnt.size() * sizeof(double), hipMemcpyDeviceToHost, st), "hipMemcpy(counts)");
        hk(hipStreamSynchronize(st), "sync");      // (iv and cnt live until here)
    }
    for (size_t s = 0; s < ns; ++s)
        for (size_t j = 0; j < npl; ++j) std::copy(cnt.begin() + (s * np + j) * nbins, cnt.begin() + (s * np + j + 1) * nbins, pdf + idx[s] * ldf + j * (nbins + 2));
}

// ---- PDF2V2D on the host (utils/pdfs.f90:215-322), plane j or the volume (j = ny); pdf: nb1*nb2 + 2 + 2*nb1 ----------------------------------------
void host_pdf2v(const Box &B, int j, const double *u, const double *v, int nb1, int nb2, double *pdf) {
    const int nb = nb1 * nb2;
    double umin = u[j < B.ny ? (size_t)j * B.nx : 0], umax = umin;
    for_plane(B, j, [&](size_t i) {
        umin = u[i] < umin ? u[i] : umin;
        umax = u[i] > umax ? u[i] : umax;
    });
    const double ustep = pdf_step(umin, umax, nb1, pdf + nb, pdf + nb + 1);
    std::vector<double> vmin(nb1, PDF_BIG), vmax(nb1, -PDF_BIG), vstep(nb1);
    for_plane(B, j, [&](size_t i) {
        const int up = pdf_bin(u[i], umin, ustep, nb1, false);
        if (up < 0 || up >= nb1) return;
        vmin[up] = v[i] < vmin[up] ? v[i] : vmin[up];
        vmax[up] = v[i] > vmax[up] ? v[i] : vmax[up];
    });
    for (int up = 0; up < nb1; ++up) vstep[up] = pdf_step(vmin[up], vmax[up], nb2, pdf + nb + 2 + up, pdf + nb + 2 + nb1 + up);
    for_plane(B, j, [&](size_t i) {
        const int up = pdf_bin(u[i], umin, ustep, nb1, false);
        if (up < 0 || up >= nb1) return;
        const int vp = pdf_bin(v[i], vmin[up], vstep[up], nb2, false);
        if (vp >= 0 && vp < nb2) pdf[vp * nb1 + up] += 1.0;
    });
}

}  // namespace

extern "C" {

int tlab_pdf_minmax_planes(int nx, int ny, int nz, int nv, const double *const *u, int igate, const signed char *gate, double *umin, double *umax) {
    (void)tlab_internal_deferred_flush();
    return catch_fail([&] {
        const char *who = "tlab_pdf_minmax_planes";
        const Box B = check_box(who, nx, ny, nz, nv, u, igate, gate);
        if (!umin || !umax) throw Fail(TLAB_EINVAL, std::string(who) + ": a null pointer");
        std::vector<int> idx(nv);
        for (int v = 0; v < nv; ++v) idx[v] = v;
        std::vector<double> mm;
        minmax_pass(B, u, idx, mm);
        for (size_t i = 0; i < (size_t)nv * (ny + 1); ++i) { umin[i] = mm[2 * i]; umax[i] = mm[2 * i + 1]; }
    }, TLAB_EINVAL);
}

int tlab_pdf_histogram_planes(int nx, int ny, int nz, int nv, int nbins, const int *ilim, const double *umin, const double *umax,
                              const double *const *u, int igate, const signed char *gate, double *pdf) {
    (void)tlab_internal_deferred_flush();
    return catch_fail([&] {
        const char *who = "tlab_pdf_histogram_planes";
        check_bins(who, nbins);
        const Box B = check_box(who, nx, ny, nz, nv, u, igate, gate);
        if (!ilim || !umin || !umax || !pdf) throw Fail(TLAB_EINVAL, std::string(who) + ": a null pointer");
        const size_t np = (size_t)ny + 1;
        std::vector<int> idx(nv);
        std::vector<char> ext(nv);
        for (int v = 0; v < nv; ++v) { idx[v] = v; ext[v] = ilim[v] == 0; }
        hist_pass(B, u, idx, nbins, ext, std::vector<double>(umin, umin + nv * np), std::vector<double>(umax, umax + nv * np), pdf, np * (nbins + 2));
    }, TLAB_EINVAL);
}

int tlab_pdf1v_n(int nx, int ny, int nz, int nv, int nbins, const int *ibc, const double *umin, const double *umax, const double *const *u,
                 int igate, const signed char *gate, double *pdf) {
    (void)tlab_internal_deferred_flush();
    return catch_fail([&] {
        const char *who = "tlab_pdf1v_n";
        check_bins(who, nbins);
        const Box B = check_box(who, nx, ny, nz, nv, u, igate, gate);
        if (!ibc || !pdf) throw Fail(TLAB_EINVAL, std::string(who) + ": a null pointer");
        const size_t np = (size_t)ny + 1, npl = ny > 1 ? np : 1, ldf = np * (nbins + 2);
        std::vector<int> all(nv), local, analysed;
        for (int v = 0; v < nv; ++v) {
            if (ibc[v] < 0 || ibc[v] > 5) throw Fail(TLAB_EINVAL, std::string(who) + ": ibc must be 0 to 5");
            if (ibc[v] == 0 && (!umin || !umax)) throw Fail(TLAB_EINVAL, std::string(who) + ": ibc = 0 needs umin and umax");
            all[v] = v;
            if (ibc[v] >= 1) local.push_back(v);
            if (ibc[v] >= 2) analysed.push_back(v);
        }
        // pass 1: the local intervals
        std::vector<double> mm;
        minmax_pass(B, u, local, mm);
        // pass 2: every field on its first interval
        std::vector<double> lo((size_t)nv * np), hi((size_t)nv * np);
        std::vector<char> ext(nv);
        for (size_t s = 0, l = 0; s < (size_t)nv; ++s) {
            ext[s] = ibc[s] == 0;
            for (size_t j = 0; j < np; ++j) {
                lo[s * np + j] = ext[s] ? umin[s] : mm[(l * np + j) * 2];
                hi[s * np + j] = ext[s] ? umax[s] : mm[(l * np + j) * 2 + 1];
            }
            if (!ext[s]) ++l;
        }
        hist_pass(B, u, all, nbins, ext, lo, hi, pdf, ldf);
        // pass 3: PDF_ANALIZE of every plane (statistics/pdf.f90:60-68, :79-87), then the histogram on its interval as an external one
        if (analysed.empty()) return;
        const size_t na = analysed.size();
        lo.assign(na * np, 0.0); hi.assign(na * np, 0.0);
        for (size_t s = 0; s < na; ++s)
            for (size_t j = 0; j < npl; ++j) {
                int nplim = 0;
                pdf_analize(ibc[analysed[s]] - 2, nbins, pdf + analysed[s] * ldf + j * (nbins + 2), &lo[s * np + j], &hi[s * np + j], 1.0e-4, &nplim);
            }
        hist_pass(B, u, analysed, nbins, std::vector<char>(na, 1), lo, hi, pdf, ldf);
    }, TLAB_EINVAL);
}

int tlab_pdf_analize(int ibc, int nbins, const double *pdf, double *umin, double *umax, double plim, int *nplim) {
    return catch_fail([&] {
        if (nbins < 1 || !pdf || !umin || !umax || !nplim) throw Fail(TLAB_EINVAL, "tlab_pdf_analize: nbins < 1 or a null pointer");
        pdf_analize(ibc, nbins, pdf, umin, umax, plim, nplim);
    }, TLAB_EINVAL);
}

int tlab_pdf2v(int nx, int ny, int nz, const int *nbins, const double *u, const double *v, double *pdf) {
    (void)tlab_internal_deferred_flush();
    return catch_fail([&] {
        const char *who = "tlab_pdf2v";
        if (!nbins || nbins[0] < 1 || nbins[1] < 1) throw Fail(TLAB_EINVAL, std::string(who) + ": nbins must be at least 1");
        check_bins(who, (long long)nbins[0] * nbins[1]);
        const int nb1 = nbins[0], nb2 = nbins[1], nb = nb1 * nb2;
        if (nb1 > PDF_LDS_WORDS / 8) throw Fail(TLAB_EINVAL, std::string(who) + ": nbins(1) must be at most " + std::to_string(PDF_LDS_WORDS / 8));
        const double *f[2] = {u, v};
        const Box B = check_box(who, nx, ny, nz, 2, f, 0, nullptr);
        if (!pdf) throw Fail(TLAB_EINVAL, std::string(who) + ": a null pointer");
        const size_t np = (size_t)ny + 1, npl = ny > 1 ? np : 1, ld = (size_t)nb + 2 + 2 * nb1;
        std::fill(pdf, pdf + np * ld, 0.0);
        if (!B.dev) {
            for (size_t j = 0; j < npl; ++j) host_pdf2v(B, (int)j, u, v, nb1, nb2, pdf + j * ld);
            return;
        }
        // pass 1: min / max of u
        std::vector<double> mm;
        minmax_pass(B, f, std::vector<int>{0}, mm);
        std::vector<double> iv(np * 2, 1.0), rng(np * nb1 * 2), viv(np * nb1 * 2, 1.0), cnt(np * nb, 0.0);
        for (size_t j = 0; j < npl; ++j) {
            iv[2 * j] = mm[2 * j];
            iv[2 * j + 1] = pdf_step(mm[2 * j], mm[2 * j + 1], nb1, pdf + j * ld + nb, pdf + j * ld + nb + 1);
        }
        // pass 2: min / max of v in every u-bin
        hipStream_t st = tlab_current_stream();
        const PdfFields F = group(B, f, std::vector<int>{0, 1}, 0);
        const size_t nchunks = pdf_chunks(nz);
        const size_t o_viv = up16(iv.size() * 8), o_rng = o_viv + up16(viv.size() * 8), o_pdf = o_rng + up16(rng.size() * 8),
                     o_vp = o_pdf + up16(cnt.size() * 8), o_part = o_vp + up16(std::max((size_t)ny * nb * 8, (size_t)ny * nb1 * 2 * 8));
        char *buf = scratch(o_part + up16(std::max(nchunks * ny * 2 * nb1 * 2 * 8, nchunks * ny * 2 * nb * 4)));
        double *div = (double *)buf, *dviv = (double *)(buf + o_viv), *drng = (double *)(buf + o_rng), *dpdf = (double *)(buf + o_pdf);
        hk(hipMemcpyAsync(div, iv.data(), iv.size() * sizeof(double), hipMemcpyHostToDevice, st), "hipMemcpy(intervals)");
        hk(launch_pdf2v_range(F, nb1, div, (double *)(buf + o_part), (double *)(buf + o_vp), drng, st), "k_pdf2v_range");
        hk(hipMemcpyAsync(rng.data(), drng, rng.size() * sizeof(double), hipMemcpyDeviceToHost, st), "hipMemcpy(ranges)");
        hk(hipStreamSynchronize(st), "sync");
        for (size_t j = 0; j < npl; ++j)
            for (int up = 0; up < nb1; ++up) {
                const size_t e = (j * nb1 + up) * 2;
                viv[e] = rng[e];
                viv[e + 1] = pdf_step(rng[e], rng[e + 1], nb2, pdf + j * ld + nb + 2 + up, pdf + j * ld + nb + 2 + nb1 + up);
            }
        // pass 3: the joint histogram
        hk(hipMemcpyAsync(dviv, viv.data(), viv.size() * sizeof(double), hipMemcpyHostToDevice, st), "hipMemcpy(v intervals)");
        hk(launch_pdf2v_hist(F, nb1, nb2, div, dviv, (unsigned *)(buf + o_part), (unsigned long long *)(buf + o_vp), dpdf, st), "k_pdf2v_hist");
        hk(hipMemcpyAsync(cnt.data(), dpdf, cnt.size() * sizeof(double), hipMemcpyDeviceToHost, st), "hipMemcpy(counts)");
        hk(hipStreamSynchronize(st), "sync");
        for (size_t j = 0; j < npl; ++j) std::copy(cnt.begin() + j * nb, cnt.begin() + (j + 1) * nb, pdf + j * ld);
    }, TLAB_EINVAL);
}

int tlab_gate_threshold(const double *a, long long n, double thr, signed char *gate) {
    (void)tlab_internal_deferred_flush();
    return catch_fail([&] {
        if (!a || !gate || n < 1) throw Fail(TLAB_EINVAL, "tlab_gate_threshold: n < 1 or a null pointer");
        if (on_device("tlab_gate_threshold", {a, gate})) hk(launch_gate_threshold(a, n, thr, gate, tlab_current_stream()), "k_gate_threshold");
        else
            for (long long i = 0; i < n; ++i) gate[i] = a[i] > thr ? 1 : 0;
    }, TLAB_EINVAL);
}

// INTER_N_XZ (statistics/avg_xz.f90:109-153, without its file) over INTER1V2D (utils/averages.f90:214-239): a count is exact and so is the
// reference's sum of 1.0_wp, so both kinds give the reference's bits
int tlab_inter_n_xz(int nx, int ny, int nz, int np, const signed char *gate, double *inter) {
    (void)tlab_internal_deferred_flush();
    return catch_fail([&] {
        const char *who = "tlab_inter_n_xz";
        if (nx < 1 || ny < 1 || nz < 1) throw Fail(TLAB_EINVAL, std::string(who) + ": nx, ny, nz must be at least 1");
        if (np < 1 || np > GATE_MAX_LEVELS) throw Fail(TLAB_EINVAL, std::string(who) + ": np must be 1 to " + std::to_string(GATE_MAX_LEVELS));
        if (!gate || !inter) throw Fail(TLAB_EINVAL, std::string(who) + ": a null pointer");
        const Box B{who, on_device(who, {gate}), nx, ny, nz, 0, gate};
        const double denom = (double)((long long)nx * nz);
        if (!B.dev) {
            for (int j = 0; j < ny; ++j)
                for (int ip = 1; ip <= np; ++ip) {
                    double avg = 0.0;
                    for_plane(B, j, [&](size_t i) { if (gate[i] == ip) avg = avg + 1.0; });
                    inter[(size_t)(ip - 1) * ny + j] = avg / denom;
                }
            return;
        }
        hipStream_t st = tlab_current_stream();
        const size_t nout = (size_t)ny * np, o_cnt = up16(nout * sizeof(double));
        char *buf = scratch(o_cnt + up16((size_t)pdf_chunks(nz) * nout * sizeof(unsigned)));
        hk(launch_gate_count(gate, nx, ny, nz, np, (unsigned *)(buf + o_cnt), (double *)buf, st), "k_gate_count");
        hk(hipMemcpyAsync(inter, buf, nout * sizeof(double), hipMemcpyDeviceToHost, st), "hipMemcpy(intermittency)");
        hk(hipStreamSynchronize(st), "sync");
    }, TLAB_EINVAL);
}

}  // extern "C"

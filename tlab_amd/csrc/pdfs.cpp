// C ABI of the plane PDFs (include/tlab_amd.h): tlab_pdf1v_n (PDF1V_N, statistics/pdf.f90:14-91, without its file), its two passes on their own
// tlab_pdf_minmax_planes / tlab_pdf_histogram_planes, tlab_pdf_analize (PDF_ANALIZE, host arithmetic), tlab_pdf2v (PDF2V, :123-159) and
// tlab_gate_threshold, and the intermittency factors of a gate, tlab_inter_n_xz (INTER_N_XZ, statistics/avg_xz.f90:109-153).  Device arrays take the kernels of pdfs.hip, host arrays the reference's loops below; a host array never reaches a kernel, a
// device array is never read by the host.  The bin of a point, the step of an interval and PDF_ANALIZE are those of pdfs_host.hpp on both sides;
// every interval bound is computed HERE, on the host, for both kinds of array.  From stats_common.hpp: on_device, Scratch with up16, Box, check_box,
// for_plane, group, minmax_pass and joint_intervals (the first two passes of tlab_pdf2v on device arrays).
#include "../../include/tlab_amd.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "driver_common.hpp"
#include "kernels.hpp"
#include "pdfs_host.hpp"
#include "stats_common.hpp"

#pragma clang fp contract(off)      // every operation below stays as written

using namespace tlab;

namespace {

Scratch g_scratch("hipMalloc(plane PDFs)");      // the device scratch of one pass

void check_bins(const char *who, long long nbins) {
    if (nbins < 1 || nbins > PDF_MAX_BINS) throw Fail(TLAB_EINVAL, std::string(who) + ": the number of bins must be 1 to " + std::to_string(PDF_MAX_BINS));
}

// ---- the reference's loops (host arrays) ---------------------------------------------------------------------------------------------------------
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
// The histograms of the fields u[idx.size()] on the intervals lo, hi [idx.size()][ny + 1] (the volume's as plane ny), ext[s]: external (a point
// outside is dropped).  Writes the whole of pdf(nbins + 2, ny + 1) of field u[s] at pdf + idx[s] * ldf: counts and the two centres; with ny == 1
// the last plane is zero.  One synchronisation.
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
        for (size_t s = 0; s < ns; ++s) host_hist(B, u[s], nbins, ext[s] != 0, iv.data() + s * np * 2, cnt.data() + s * np * nbins);
    } else {
        hipStream_t st = tlab_current_stream();
        const size_t ncnt = (size_t)PDF_FIELDS_PER_LAUNCH * pdf_chunks(B.nz) * B.ny * 2 * nbins, nvp = (size_t)PDF_FIELDS_PER_LAUNCH * B.ny * nbins;
        const size_t o_pdf = up16(iv.size() * 8), o_vp = o_pdf + up16(cnt.size() * 8), o_cnt = o_vp + up16(nvp * 8);
        char *buf = g_scratch.bytes(o_cnt + up16(ncnt * 4));
        double *div = (double *)buf, *dpdf = (double *)(buf + o_pdf);
        hk(hipMemcpyAsync(div, iv.data(), iv.size() * sizeof(double), hipMemcpyHostToDevice, st), "hipMemcpy(intervals)");
        for (size_t v0 = 0; v0 < ns; v0 += PDF_FIELDS_PER_LAUNCH) {
            const PdfFields F = group(B, u, v0, ns);
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
        std::vector<double> mm;
        minmax_pass(B, g_scratch, u, nv, mm);
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
        std::vector<int> all(nv), analysed;
        std::vector<const double *> local, ua;      // the fields with a local interval, the fields of analysed
        for (int v = 0; v < nv; ++v) {
            if (ibc[v] < 0 || ibc[v] > 5) throw Fail(TLAB_EINVAL, std::string(who) + ": ibc must be 0 to 5");
            if (ibc[v] == 0 && (!umin || !umax)) throw Fail(TLAB_EINVAL, std::string(who) + ": ibc = 0 needs umin and umax");
            all[v] = v;
            if (ibc[v] >= 1) local.push_back(u[v]);
            if (ibc[v] >= 2) { analysed.push_back(v); ua.push_back(u[v]); }
        }
        // pass 1: the local intervals
        std::vector<double> mm;
        minmax_pass(B, g_scratch, local.data(), local.size(), mm);
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
        hist_pass(B, ua.data(), analysed, nbins, std::vector<char>(na, 1), lo, hi, pdf, ldf);
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
        // passes 1 and 2: min / max of u, then of v in every u-bin
        std::vector<double> iv, viv, cnt(np * nb, 0.0);
        joint_intervals(B, g_scratch, f, nb1, nb2, pdf, ld, iv, viv);
        // pass 3: the joint histogram (the u-intervals go to the device once more: the scratch of pass 2 is not kept)
        hipStream_t st = tlab_current_stream();
        const size_t o_viv = up16(iv.size() * 8), o_pdf = o_viv + up16(viv.size() * 8), o_vp = o_pdf + up16(cnt.size() * 8),
                     o_part = o_vp + up16((size_t)ny * nb * 8);
        char *buf = g_scratch.bytes(o_part + up16((size_t)pdf_chunks(nz) * ny * 2 * nb * 4));
        double *div = (double *)buf, *dviv = (double *)(buf + o_viv), *dpdf = (double *)(buf + o_pdf);
        hk(hipMemcpyAsync(div, iv.data(), iv.size() * sizeof(double), hipMemcpyHostToDevice, st), "hipMemcpy(intervals)");
        hk(hipMemcpyAsync(dviv, viv.data(), viv.size() * sizeof(double), hipMemcpyHostToDevice, st), "hipMemcpy(v intervals)");
        hk(launch_pdf2v_hist(group(B, f, 0, 2), nb1, nb2, div, dviv, (unsigned *)(buf + o_part), (unsigned long long *)(buf + o_vp), dpdf, st), "k_pdf2v_hist");
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
        const Box B{on_device(who, {gate}), nx, ny, nz, 0, gate};
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
        char *buf = g_scratch.bytes(o_cnt + up16((size_t)pdf_chunks(nz) * nout * sizeof(unsigned)));
        hk(launch_gate_count(gate, nx, ny, nz, np, (unsigned *)(buf + o_cnt), (double *)buf, st), "k_gate_count");
        hk(hipMemcpyAsync(inter, buf, nout * sizeof(double), hipMemcpyDeviceToHost, st), "hipMemcpy(intermittency)");
        hk(hipStreamSynchronize(st), "sync");
    }, TLAB_EINVAL);
}

}  // extern "C"

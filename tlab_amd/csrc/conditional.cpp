// C ABI of the conditional statistics (tlab_amd_conditional.h): the partition tlab_gate_levels, tlab_gate_flux and tlab_dns_gate (FI_GATE,
// mappings/fi_gate.f90), the gated moments tlab_avg_n_xz (AVG_N_XZ, statistics/avg_xz.f90:10-70, without its file) with tlab_raw_to_central, and the
// conditional averages tlab_cavg1v_n, tlab_cavg2v (statistics/cavg.f90 over the a, avg arguments of module PDFS).  Device arrays take the kernels of
// conditional.hip, host arrays the reference's loops below in the reference's order; a host array never reaches a kernel, a device array is never
// read by the host.  The level and the bin of a point, the integer power and RAW_TO_CENTRAL are those of conditional_host.hpp / pdfs_host.hpp on
// both sides; every interval bound and every division is computed HERE, on the host, for both kinds of array.  From stats_common.hpp: on_device,
// Scratch with up16, Box, check_box, for_plane, group, minmax_pass (the intervals of tlab_cavg1v_n are those of tlab_pdf1v_n) and joint_intervals.
#include "tlab_amd_conditional.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "conditional_host.hpp"
#include "dns_state.hpp"
#include "driver_common.hpp"
#include "kernels.hpp"
#include "stats_common.hpp"

#pragma clang fp contract(off)      // every operation below stays as written

using namespace tlab;

namespace {

Scratch g_scratch("hipMalloc(conditional statistics)");      // the device scratch of one pass
constexpr size_t PARTIAL_BYTES = (size_t)256 << 20;      // what the partial tables of one launch may take: fewer fields per launch above it

// The sums of a and the counts per bin of nv fields on the intervals iv [nv][ny + 1][2] = (umin, ustep) (nb2 == 0), or of the pair (u[0], v2) with
// the v-intervals viv [ny + 1][nb1][2] of every u-bin (nb2 > 0): sum, cnt [nv][ny + 1][nbins], the volume as plane ny (zero when ny == 1)
void cavg_pass(const Box &B, const double *const *u, size_t nv, const double *v2, const double *a, int nb1, int nb2, const std::vector<char> &ext,
               const std::vector<double> &iv, const std::vector<double> &viv, std::vector<double> &sum, std::vector<double> &cnt) {
    const size_t np = (size_t)B.ny + 1, npl = B.ny > 1 ? np : 1, nb = (size_t)nb1 * (nb2 > 0 ? nb2 : 1);
    sum.assign(nv * np * nb, 0.0);
    cnt.assign(nv * np * nb, 0.0);
    if (!B.dev) {      // utils/pdfs.f90:76-90, :172-189, :283-300: the sum goes to the bin the count goes to, in the order of the points
        for (size_t v = 0; v < nv; ++v)
            for (size_t j = 0; j < npl; ++j) {
                double *s = sum.data() + (v * np + j) * nb, *c = cnt.data() + (v * np + j) * nb;
                const double umin = iv[(v * np + j) * 2], ustep = iv[(v * np + j) * 2 + 1];
                for_plane(B, (int)j, [&](size_t i) {
                    if (B.gate && B.gate[i] != B.igate) return;
                    int b = pdf_bin(u[v][i], umin, ustep, nb1, ext[v] != 0);
                    if (b < 0 || b >= nb1) return;
                    if (nb2 > 0) {
                        const int vp = pdf_bin(v2[i], viv[(j * nb1 + b) * 2], viv[(j * nb1 + b) * 2 + 1], nb2, false);
                        if (vp < 0 || vp >= nb2) return;
                        b = vp * nb1 + b;
                    }
                    c[b] = c[b] + 1.0;
                    s[b] = s[b] + a[i];
                });
            }
        return;
    }
    hipStream_t st = tlab_current_stream();
    const size_t nchunks = pdf_chunks(B.nz), part1 = nchunks * B.ny * 2 * nb;      // partial entries of one field
    const size_t per = std::max<size_t>(1, std::min<size_t>(PDF_FIELDS_PER_LAUNCH, PARTIAL_BYTES / (part1 * 12)));
    const size_t o_viv = up16(iv.size() * 8), o_sum = o_viv + up16(viv.size() * 8), o_cnt = o_sum + up16(sum.size() * 8),
                 o_vs = o_cnt + up16(cnt.size() * 8), o_vc = o_vs + up16(per * B.ny * nb * 8), o_ps = o_vc + up16(per * B.ny * nb * 8),
                 o_pc = o_ps + up16(per * part1 * 8);
    char *buf = g_scratch.bytes(o_pc + up16(per * part1 * 4));
    double *div = (double *)buf, *dviv = (double *)(buf + o_viv), *dsum = (double *)(buf + o_sum), *dcnt = (double *)(buf + o_cnt);
    hk(hipMemcpyAsync(div, iv.data(), iv.size() * sizeof(double), hipMemcpyHostToDevice, st), "hipMemcpy(intervals)");
    if (nb2 > 0) hk(hipMemcpyAsync(dviv, viv.data(), viv.size() * sizeof(double), hipMemcpyHostToDevice, st), "hipMemcpy(v intervals)");
    if (B.ny == 1) {      // no volume plane: nothing writes it
        hk(hipMemsetAsync(dsum, 0, sum.size() * 8, st), "hipMemset");
        hk(hipMemsetAsync(dcnt, 0, cnt.size() * 8, st), "hipMemset");
    }
    for (size_t v0 = 0; v0 < nv; v0 += per) {
        const PdfFields F = group(B, u, v0, nv, per);
        unsigned em = 0u;
        for (int i = 0; i < F.nv; ++i) em |= ext[v0 + i] ? 1u << i : 0u;
        hk(launch_cavg_sum(F, v2, a, nb1, nb2, em, div + v0 * np * 2, nb2 > 0 ? dviv : nullptr, (double *)(buf + o_ps), (unsigned *)(buf + o_pc),
                           (double *)(buf + o_vs), (unsigned long long *)(buf + o_vc), dsum + v0 * np * nb, dcnt + v0 * np * nb, st), "k_cavg_sum");
    }
    hk(hipMemcpyAsync(sum.data(), dsum, sum.size() * sizeof(double), hipMemcpyDeviceToHost, st), "hipMemcpy(sums)");
    hk(hipMemcpyAsync(cnt.data(), dcnt, cnt.size() * sizeof(double), hipMemcpyDeviceToHost, st), "hipMemcpy(counts)");
    hk(hipStreamSynchronize(st), "sync");      // (iv and viv live until here)
}

void check_cavg_bins(const char *who, long long nbins) {
    if (nbins < 1 || nbins > CAVG_MAX_BINS)
        throw Fail(TLAB_EINVAL, std::string(who) + ": the number of bins must be 1 to CAVG_MAX_BINS = " + std::to_string(CAVG_MAX_BINS));
}

// avg(up) = avg(up)/pdf(up) where pdf(up) > 0 (utils/pdfs.f90:103-110): one division per bin
void divide(const double *sum, const double *cnt, size_t nb, double *avg) {
    for (size_t b = 0; b < nb; ++b) avg[b] = cnt[b] > 0.0 ? sum[b] / cnt[b] : sum[b];
}

}  // namespace

extern "C" {

int tlab_gate_levels(const double *a, long long n, int igate_size, const double *thr, signed char *gate) {
    (void)tlab_internal_deferred_flush();
    return catch_fail([&] {
        const char *who = "tlab_gate_levels";
        if (!a || !gate || n < 1) throw Fail(TLAB_EINVAL, std::string(who) + ": n < 1 or a null pointer");
        if (igate_size < 1 || igate_size > GATE_MAX_LEVELS)
            throw Fail(TLAB_EINVAL, std::string(who) + ": igate_size must be 1 to " + std::to_string(GATE_MAX_LEVELS));
        if (igate_size > 1 && !thr) throw Fail(TLAB_EINVAL, std::string(who) + ": no thresholds");
        if (on_device(who, {a, gate})) hk(launch_gate_levels(a, n, igate_size, thr, gate, tlab_current_stream()), "k_gate_levels");
        else
            for (long long i = 0; i < n; ++i) gate[i] = gate_level(a[i], thr, igate_size);
    }, TLAB_EINVAL);
}

int tlab_gate_flux(const double *a, const double *v, long long n, signed char *gate) {
    (void)tlab_internal_deferred_flush();
    return catch_fail([&] {
        const char *who = "tlab_gate_flux";
        if (!a || !v || !gate || n < 1) throw Fail(TLAB_EINVAL, std::string(who) + ": n < 1 or a null pointer");
        if (on_device(who, {a, v, gate})) hk(launch_gate_flux(a, v, n, gate, tlab_current_stream()), "k_gate_flux");
        else
            for (long long i = 0; i < n; ++i) gate[i] = gate_quadrant(a[i], v[i]);
    }, TLAB_EINVAL);
}

int tlab_dns_gate(tlab_dns_t d, int opt_cond, int opt_cond_relative, int opt_cond_scal, int igate_size, const double *gate_threshold,
                  double *const *q, double *const *s, double *const *txc, signed char *gate) {
    (void)tlab_internal_deferred_flush();
    return catch_fail([&] {
        const char *who = "tlab_dns_gate";
        if (opt_cond == 8) throw Fail(TLAB_EUNSUPPORTED, std::string(who) + ": opt_cond = 8 (potential vorticity) needs FI_CURL, which is not built");
        if (opt_cond < 2 || opt_cond > 8) throw Fail(TLAB_EINVAL, std::string(who) + ": opt_cond must be 2 to 7 (1 reads the gate from a file: the host's)");
        if (!d || !q || !gate) throw Fail(TLAB_EINVAL, std::string(who) + ": a null pointer");
        const bool scal = opt_cond == 2 || opt_cond == 4 || opt_cond == 6 || opt_cond == 7;
        if (scal && (!s || opt_cond_scal < 1 || opt_cond_scal > d->scal_arrays()))
            throw Fail(TLAB_EINVAL, std::string(who) + ": opt_cond_scal must be 1 to the number of scalar arrays");
        if (opt_cond != 7) {
            if (igate_size < 1 || igate_size > GATE_MAX_LEVELS)
                throw Fail(TLAB_EINVAL, std::string(who) + ": igate_size must be 1 to " + std::to_string(GATE_MAX_LEVELS));
            if (igate_size > 1 && !gate_threshold) throw Fail(TLAB_EINVAL, std::string(who) + ": no thresholds");
        }
        const int ntxc = opt_cond == 3 ? 7 : opt_cond == 4 ? 2 : opt_cond >= 6 ? 1 : 0;
        if (ntxc > 0 && !txc) throw Fail(TLAB_EINVAL, std::string(who) + ": a null pointer");
        for (int i = 0; i < ntxc; ++i)
            if (!txc[i]) throw Fail(TLAB_EINVAL, std::string(who) + ": a null txc array");
        for (int i = 0; i < 3; ++i)
            if ((opt_cond == 3 || (i == 1 && (opt_cond == 5 || opt_cond == 7))) && !q[i]) throw Fail(TLAB_EINVAL, std::string(who) + ": a null velocity");
        const int nx = d->nx, ny = d->ny, nz = d->nz;
        const long long n = (long long)nx * ny * nz;
        const double *sc = scal ? s[opt_cond_scal - 1] : nullptr, *ind = nullptr;      // the indicator: txc(:, 1) of the reference, or the field itself
        if (scal && !sc) throw Fail(TLAB_EINVAL, std::string(who) + ": a null scalar");
        if (opt_cond == 2) ind = sc;
        else if (opt_cond == 5) ind = q[1];
        else if (opt_cond == 3) { ok(tlab_fi_vorticity(d, q[0], q[1], q[2], txc[0], txc + 1), "FI_VORTICITY"); ind = txc[0]; }
        else if (opt_cond == 4) { ok(tlab_fi_gradient(d, sc, txc[0], txc[1]), "FI_GRADIENT"); ind = txc[0]; }
        else {      // FI_FLUCTUATION_INPLACE of a copy: out = in - mean(j)
            std::vector<double> mean(ny);
            ok(tlab_avg_ik_v(nx, ny, nz, 1, &sc, mean.data(), ny), "AVG_IK_V");
            ok(tlab_fluctuation(nx, ny, nz, sc, mean.data(), txc[0]), "FI_FLUCTUATION");
            ind = txc[0];
        }
        if (opt_cond == 7) { ok(tlab_gate_flux(ind, q[1], n, gate)); return; }
        std::vector<double> thr(gate_threshold, gate_threshold + (igate_size - 1));
        if (opt_cond_relative == 1) {
            double umin = 0.0, umax = 0.0;
            ok(tlab_minmax(d, ind, nx, ny, nz, &umin, &umax), "MINMAX");
            for (double &t : thr) t = t * (umax - umin);
        }
        ok(tlab_gate_levels(ind, n, igate_size, thr.data(), gate));
    }, TLAB_EINVAL);
}

int tlab_raw_to_central(int nm, double *moments) {
    return catch_fail([&] {
        if (nm < 1 || nm > COND_MAX_MOMENTS || !moments)
            throw Fail(TLAB_EINVAL, "tlab_raw_to_central: nm must be 1 to " + std::to_string(COND_MAX_MOMENTS) + ", moments not null");
        raw_to_central(nm, moments);
    }, TLAB_EINVAL);
}

int tlab_avg_n_xz(int nx, int ny, int nz, int nv, int nm, const double *const *u, int np, const signed char *gate, double *avg, double *sums,
                  long long *nsample) {
    (void)tlab_internal_deferred_flush();
    return catch_fail([&] {
        const char *who = "tlab_avg_n_xz";
        if (nm < 1 || nm > COND_MAX_MOMENTS) throw Fail(TLAB_EINVAL, std::string(who) + ": nm must be 1 to " + std::to_string(COND_MAX_MOMENTS));
        if (np < 0 || np > GATE_MAX_LEVELS) throw Fail(TLAB_EINVAL, std::string(who) + ": np must be 0 to " + std::to_string(GATE_MAX_LEVELS));
        if (np > 0 && !gate) throw Fail(TLAB_EINVAL, std::string(who) + ": np > 0 needs a gate");
        if (!avg && !sums && !nsample) throw Fail(TLAB_EINVAL, std::string(who) + ": no output");
        const Box B = check_box(who, nx, ny, nz, nv, u, np > 0 ? 1 : 0, gate, nullptr);      // (igate here only says: the gate is read)
        const size_t L = (size_t)std::max(np, 1), nout = (size_t)ny * nm * nv * L;
        std::vector<double> S(nout, 0.0);
        std::vector<long long> N((size_t)ny * L, 0);
        if (!B.dev) {      // AVG1V2D / AVG1V2D1G: k outer, i inner, one running sum per (plane, field, level, moment)
            for (size_t l = 0; l < L; ++l)
                for (int v = 0; v < nv; ++v)
                    for (int j = 0; j < ny; ++j) {
                        double acc[COND_MAX_MOMENTS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
                        long long ns = 0;
                        for_plane(B, j, [&](size_t i) {
                            if (B.gate && B.gate[i] != (signed char)(l + 1)) return;
                            for (int m = 1; m <= nm; ++m) acc[m - 1] = acc[m - 1] + ipow(u[v][i], m);
                            ns = ns + 1;
                        });
                        for (int m = 0; m < nm; ++m) S[((l * nv + v) * nm + m) * ny + j] = acc[m];
                        N[l * ny + j] = ns;
                    }
        } else {
            hipStream_t st = tlab_current_stream();
            const size_t npart = (size_t)PDF_FIELDS_PER_LAUNCH * pdf_chunks(nz) * ny * COND_LEVELS_PER_LAUNCH * gated_moments_width(nm),
                         ncnt = (size_t)pdf_chunks(nz) * ny * COND_LEVELS_PER_LAUNCH;
            const size_t o_n = up16(nout * 8), o_part = o_n + up16(N.size() * 8), o_cnt = o_part + up16(npart * 8);
            char *buf = g_scratch.bytes(o_cnt + up16(ncnt * 4));
            for (size_t v0 = 0; v0 < (size_t)nv; v0 += PDF_FIELDS_PER_LAUNCH)
                for (size_t g0 = 1; g0 <= L; g0 += COND_LEVELS_PER_LAUNCH)
                    hk(launch_gated_moments(group(B, u, v0, nv), nm, (int)g0, (int)L, (int)v0, nv, (double *)(buf + o_part),
                                            (unsigned *)(buf + o_cnt), (double *)buf, (long long *)(buf + o_n), st), "k_gated_moments");
            hk(hipMemcpyAsync(S.data(), buf, nout * 8, hipMemcpyDeviceToHost, st), "hipMemcpy(sums)");
            hk(hipMemcpyAsync(N.data(), buf + o_n, N.size() * 8, hipMemcpyDeviceToHost, st), "hipMemcpy(counts)");
            hk(hipStreamSynchronize(st), "sync");
        }
        if (sums) std::copy(S.begin(), S.end(), sums);
        if (nsample) std::copy(N.begin(), N.end(), nsample);
        if (!avg) return;
        // avg/real(nx*nz) (averages.f90:130) or avg/real(nsample) where nsample > 0 (:205), then RAW_TO_CENTRAL (avg_xz.f90:50)
        for (size_t l = 0; l < L; ++l)
            for (int v = 0; v < nv; ++v)
                for (int j = 0; j < ny; ++j) {
                    double mom[COND_MAX_MOMENTS];
                    const long long ns = N[l * ny + j];
                    for (int m = 0; m < nm; ++m) {
                        const double s = S[((l * nv + v) * nm + m) * ny + j];
                        mom[m] = ns > 0 ? s / (double)ns : s;
                    }
                    if (nm > 1) raw_to_central(nm, mom);
                    for (int m = 0; m < nm; ++m) avg[((l * nv + v) * nm + m) * ny + j] = mom[m];
                }
    }, TLAB_EINVAL);
}

int tlab_cavg1v_n(int nx, int ny, int nz, int nv, int nbins, const int *ibc, const double *umin, const double *umax, const double *const *u,
                  int igate, const signed char *gate, const double *a, double *avg, double *sum, double *pdf) {
    (void)tlab_internal_deferred_flush();
    return catch_fail([&] {
        const char *who = "tlab_cavg1v_n";
        check_cavg_bins(who, nbins);
        if (!ibc || !a || !avg) throw Fail(TLAB_EINVAL, std::string(who) + ": a null pointer");
        const Box B = check_box(who, nx, ny, nz, nv, u, igate, gate, a);
        const size_t np = (size_t)ny + 1, npl = ny > 1 ? np : 1, ld = np * (nbins + 2);
        std::vector<const double *> local;
        std::vector<char> ext(nv);
        for (int v = 0; v < nv; ++v) {
            ext[v] = ibc[v] == 0;      // (CAVG1V_N hands ibc to PDF1V2D as ilim: 0 the external interval, anything else the local one)
            if (ext[v] && (!umin || !umax)) throw Fail(TLAB_EINVAL, std::string(who) + ": ibc = 0 needs umin and umax");
            if (!ext[v]) local.push_back(u[v]);
        }
        std::vector<double> mm, iv((size_t)nv * np * 2, 1.0), S, C;
        minmax_pass(B, g_scratch, local.data(), local.size(), mm);
        for (double *out : {avg, sum, pdf})
            if (out) std::fill(out, out + (size_t)nv * ld, 0.0);
        for (size_t v = 0, l = 0; v < (size_t)nv; ++v) {
            for (size_t j = 0; j < npl; ++j) {
                const double lo = ext[v] ? umin[v] : mm[(l * np + j) * 2], hi = ext[v] ? umax[v] : mm[(l * np + j) * 2 + 1];
                double *p = avg + v * ld + j * (nbins + 2) + nbins;
                iv[(v * np + j) * 2] = lo;
                iv[(v * np + j) * 2 + 1] = pdf_step(lo, hi, nbins, p, p + 1);
                for (double *out : {sum, pdf})
                    if (out) std::copy(p, p + 2, out + v * ld + j * (nbins + 2) + nbins);
            }
            if (!ext[v]) ++l;
        }
        cavg_pass(B, u, nv, nullptr, a, nbins, 0, ext, iv, {}, S, C);
        for (size_t v = 0; v < (size_t)nv; ++v)
            for (size_t j = 0; j < npl; ++j) {
                const size_t in = (v * np + j) * nbins, out = v * ld + j * (nbins + 2);
                divide(S.data() + in, C.data() + in, nbins, avg + out);
                if (sum) std::copy(S.begin() + in, S.begin() + in + nbins, sum + out);
                if (pdf) std::copy(C.begin() + in, C.begin() + in + nbins, pdf + out);
            }
    }, TLAB_EINVAL);
}

int tlab_cavg2v(int nx, int ny, int nz, const int *nbins, const double *u, const double *v, const double *a, double *avg) {
    (void)tlab_internal_deferred_flush();
    return catch_fail([&] {
        const char *who = "tlab_cavg2v";
        if (!nbins || nbins[0] < 1 || nbins[1] < 1) throw Fail(TLAB_EINVAL, std::string(who) + ": nbins must be at least 1");
        check_cavg_bins(who, (long long)nbins[0] * nbins[1]);
        if (!u || !v || !a || !avg) throw Fail(TLAB_EINVAL, std::string(who) + ": a null pointer");
        const int nb1 = nbins[0], nb2 = nbins[1], nb = nb1 * nb2;
        const double *f[2] = {u, v};
        const Box B = check_box(who, nx, ny, nz, 2, f, 0, nullptr, a);
        const size_t np = (size_t)ny + 1, npl = ny > 1 ? np : 1, ld = (size_t)nb + 2 + 2 * nb1;
        std::fill(avg, avg + np * ld, 0.0);
        std::vector<double> iv, viv, S, C;
        joint_intervals(B, g_scratch, f, nb1, nb2, avg, ld, iv, viv);
        cavg_pass(B, f, 1, v, a, nb1, nb2, std::vector<char>(1, 0), iv, viv, S, C);
        for (size_t j = 0; j < npl; ++j) divide(S.data() + j * nb, C.data() + j * nb, nb, avg + j * ld);
    }, TLAB_EINVAL);
}

}  // extern "C"

// C ABI of the plane statistics (include/tlab_amd.h): tlab_avg_ik_v, tlab_avg1v2d_v, tlab_avg_moments_flow, tlab_avg_moments_scal and the gradient
// statistics tlab_avg_gradients_flow, tlab_avg_ugradp, tlab_avg_gradients_scal, tlab_avg_gradients_pass (several programs one after the other:
// the profiles of one pass are the means of the next).  Device arrays
// take the kernels of averages.hip, host arrays the loop below in the reference's order; a host array never reaches a kernel, a device array is
// never read by the host.  The programs (the terms of every output) are those of averages_host.hpp on both sides.  From stats_common.hpp:
// on_device and Scratch.
#include "../../include/tlab_amd.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "averages_host.hpp"
#include "driver_common.hpp"
#include "kernels.hpp"
#include "stats_common.hpp"

#pragma clang fp contract(off)      // every multiply and add below stays as written

using namespace tlab;

namespace {

Scratch g_scratch("hipMalloc(plane statistics)");      // partials, table of means and profile of one launch

// AVG_IK_V's loop nest for one plane (utils/averages.f90:311-320): k outer, i inner, one running sum per output, then the division
template <class P>
void host_planes(int nx, int ny, int nz, const double *const *f, const double *const *means, double *out, int ldout) {
    const double denom = (double)((long long)nx * nz);
    for (int j = 0; j < ny; ++j) {
        double m[P::NMEAN > 0 ? P::NMEAN : 1], acc[P::NOUT], x[P::NFLD];
        for (int i = 0; i < P::NMEAN; ++i) m[i] = means[i][j];
        for (int o = 0; o < P::NOUT; ++o) acc[o] = 0.0;
        for (int k = 0; k < nz; ++k) {
            const size_t row = ((size_t)k * ny + j) * nx;
            for (int i = 0; i < nx; ++i) {
                for (int c = 0; c < P::NFLD; ++c) x[c] = f[c][row + i];
                P::add(x, m, acc);
            }
        }
        for (int o = 0; o < P::NOUT; ++o) out[(size_t)o * ldout + j] = acc[o] / denom;
    }
}

// one program on its fields: f[nfld], means[nmean] (host profiles), out: nout columns ldout apart
void run(bool device, int prog, int param, int nx, int ny, int nz, const double *const *f, const double *const *means, double *out, int ldout) {
    const AvgInfo info = avg_info(prog, param);
    if (!device) {
        avg_dispatch(prog, param, [&](auto P) { host_planes<decltype(P)>(nx, ny, nz, f, means, out, ldout); });
        return;
    }
    hipStream_t st = tlab_current_stream();
    const size_t npart = (size_t)plane_moments_chunks(nz) * ny * info.nout, nmean = (size_t)info.nmean * ny, nprof = (size_t)info.nout * ny;
    double *partial = g_scratch.doubles(npart + nmean + nprof), *dmeans = partial + npart, *prof = dmeans + nmean;
    std::vector<double> hm(nmean), hp(nprof);      // (both live until the stream is synchronised below)
    if (nmean) {
        for (int i = 0; i < info.nmean; ++i) std::copy(means[i], means[i] + ny, hm.begin() + (size_t)i * ny);
        hk(hipMemcpyAsync(dmeans, hm.data(), nmean * sizeof(double), hipMemcpyHostToDevice, st), "hipMemcpy(means)");
    }
    hk(launch_plane_moments(prog, param, nx, ny, nz, f, nmean ? dmeans : nullptr, partial, prof, st), "k_plane_partial");
    hk(hipMemcpyAsync(hp.data(), prof, nprof * sizeof(double), hipMemcpyDeviceToHost, st), "hipMemcpy(profile)");
    hk(hipStreamSynchronize(st), "sync");
    for (int o = 0; o < info.nout; ++o) std::copy(hp.begin() + (size_t)o * ny, hp.begin() + (size_t)(o + 1) * ny, out + (size_t)o * ldout);
}

void check_profiles(const char *who, int nx, int ny, int nz, int ld) {
    if (nx < 1 || ny < 1 || nz < 1) throw Fail(TLAB_EINVAL, std::string(who) + ": nx, ny, nz must be at least 1");
    if (ld < ny) throw Fail(TLAB_EINVAL, std::string(who) + ": the leading dimension of the profiles is smaller than ny");
}

}  // namespace

extern "C" {

int tlab_avg_ik_v(int nx, int ny, int nz, int nf, const double *const *a, double *avg, int ldavg) {
    (void)tlab_internal_deferred_flush();
    return catch_fail([&] {
        if (nf < 1 || !a || !avg) throw Fail(TLAB_EINVAL, "tlab_avg_ik_v: nf < 1 or a null pointer");
        check_profiles("tlab_avg_ik_v", nx, ny, nz, ldavg);
        for (int f = 0; f < nf; ++f)
            if (!a[f]) throw Fail(TLAB_EINVAL, "tlab_avg_ik_v: a null array");
        const bool dev = on_device("tlab_avg_ik_v", a, nf);
        for (int f0 = 0; f0 < nf; f0 += AVG_FIELDS_PER_LAUNCH) {
            const int n = std::min(AVG_FIELDS_PER_LAUNCH, nf - f0);
            run(dev, AVG_PROG_MEANS, n, nx, ny, nz, a + f0, nullptr, avg + (size_t)f0 * ldavg, ldavg);
        }
    }, TLAB_EINVAL);
}

int tlab_avg1v2d_v(int nx, int ny, int nz, int imom, const double *a, double *avg) {
    (void)tlab_internal_deferred_flush();
    return catch_fail([&] {
        if (!a || !avg) throw Fail(TLAB_EINVAL, "tlab_avg1v2d_v: a null pointer");
        if (imom < 1 || imom > 4) throw Fail(TLAB_EINVAL, "tlab_avg1v2d_v: imom must be 1 to 4");
        check_profiles("tlab_avg1v2d_v", nx, ny, nz, ny);
        run(on_device("tlab_avg1v2d_v", &a, 1), AVG_PROG_POWER, imom, nx, ny, nz, &a, nullptr, avg, ny);
    }, TLAB_EINVAL);
}

int tlab_avg_cov2v(int nx, int ny, int nz, const double *a, const double *b, double *cov, int ldcov) {
    (void)tlab_internal_deferred_flush();
    return catch_fail([&] {
        if (!a || !b || !cov) throw Fail(TLAB_EINVAL, "tlab_avg_cov2v: a null pointer");
        check_profiles("tlab_avg_cov2v", nx, ny, nz, ldcov);
        const double *f[2] = {a, b};
        run(on_device("tlab_avg_cov2v", f, 2), AVG_PROG_COV2, 0, nx, ny, nz, f, nullptr, cov, ldcov);
    }, TLAB_EINVAL);
}

int tlab_avg_moments_flow(int nx, int ny, int nz, const double *u, const double *v, const double *w, const double *p, const double *fU,
                          const double *fV, const double *fW, const double *rP, double *out, int ldout) {
    (void)tlab_internal_deferred_flush();
    return catch_fail([&] {
        if (!u || !v || !w || !fU || !fV || !fW || !out || (p == nullptr) != (rP == nullptr))
            throw Fail(TLAB_EINVAL, "tlab_avg_moments_flow: a null pointer (p and rP may be NULL, together)");
        check_profiles("tlab_avg_moments_flow", nx, ny, nz, ldout);
        const double *f[4] = {u, v, w, p}, *m[4] = {fU, fV, fW, rP};
        run(on_device("tlab_avg_moments_flow", f, p ? 4 : 3), AVG_PROG_FLOW, p ? 1 : 0, nx, ny, nz, f, m, out, ldout);
    }, TLAB_EINVAL);
}

int tlab_avg_moments_scal(int nx, int ny, int nz, const double *s, const double *u, const double *v, const double *w, const double *p,
                          const double *fS, const double *fU, const double *fV, const double *fW, const double *rP, double *out, int ldout) {
    (void)tlab_internal_deferred_flush();
    return catch_fail([&] {
        if (!s || !u || !v || !w || !fS || !fU || !fV || !fW || !out || (p == nullptr) != (rP == nullptr))
            throw Fail(TLAB_EINVAL, "tlab_avg_moments_scal: a null pointer (p and rP may be NULL, together)");
        check_profiles("tlab_avg_moments_scal", nx, ny, nz, ldout);
        const double *f[5] = {s, u, v, w, p}, *m[5] = {fS, fU, fV, fW, rP};
        run(on_device("tlab_avg_moments_scal", f, p ? 5 : 4), AVG_PROG_SCAL, p ? 1 : 0, nx, ny, nz, f, m, out, ldout);
    }, TLAB_EINVAL);
}

// One pass of the gradient statistics: the program of pass 1-3 (flow) or 4-5 (scalar) on its own fields and means, in the program's order
// (averages_host.hpp).  A decomposed host reduces the profiles of one pass over its ranks before it hands them to the next as means.
int tlab_avg_gradients_pass(int pass, int with_p, int nx, int ny, int nz, const double *const *fields, const double *const *means, double *out,
                            int ldout) {
    (void)tlab_internal_deferred_flush();
    return catch_fail([&] {
        const char *who = "tlab_avg_gradients_pass";
        static const int progs[5] = {AVG_PROG_GRAD_FLOW1, AVG_PROG_GRAD_FLOW2, AVG_PROG_GRAD_FLOW3, AVG_PROG_GRAD_SCAL1, AVG_PROG_GRAD_SCAL2};
        if (pass < 1 || pass > 5) throw Fail(TLAB_EINVAL, std::string(who) + ": pass must be 1 to 5");
        const AvgInfo info = avg_info(progs[pass - 1], with_p ? 1 : 0);
        if (!fields || !out || (info.nmean > 0 && !means)) throw Fail(TLAB_EINVAL, std::string(who) + ": a null pointer");
        check_profiles(who, nx, ny, nz, ldout);
        for (int i = 0; i < info.nfld; ++i)
            if (!fields[i]) throw Fail(TLAB_EINVAL, std::string(who) + ": a null field");
        for (int i = 0; i < info.nmean; ++i)
            if (!means[i]) throw Fail(TLAB_EINVAL, std::string(who) + ": a null profile");
        run(on_device(who, fields, info.nfld), progs[pass - 1], with_p ? 1 : 0, nx, ny, nz, fields, means, out, ldout);
    }, TLAB_EINVAL);
}

int tlab_avg_gradients_flow(int nx, int ny, int nz, const double *const *grad, const double *u, const double *v, const double *w, const double *p,
                            const double *fU, const double *fV, const double *fW, const double *rP, const double *rU_y, const double *rV_y,
                            const double *rW_y, double *out, int ldout) {
    (void)tlab_internal_deferred_flush();
    return catch_fail([&] {
        const char *who = "tlab_avg_gradients_flow";
        if (!grad || !u || !v || !w || !fU || !fV || !fW || !rU_y || !rV_y || !rW_y || !out || (p == nullptr) != (rP == nullptr))
            throw Fail(TLAB_EINVAL, std::string(who) + ": a null pointer (p and rP may be NULL, together)");
        check_profiles(who, nx, ny, nz, ldout);
        const double *f[13] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, u, v, w, p};
        for (int i = 0; i < 9; ++i) {
            if (!grad[i]) throw Fail(TLAB_EINVAL, std::string(who) + ": a null gradient array");
            f[i] = grad[i];
        }
        const bool dev = on_device(who, f, p ? 13 : 12);
        auto col = [&](int c) { return out + (size_t)c * ldout; };
        run(dev, AVG_PROG_GRAD_FLOW1, 0, nx, ny, nz, f, nullptr, col(0), ldout);
        const double *m2[6] = {rU_y, rV_y, rW_y, col(0), col(1), col(2)};
        run(dev, AVG_PROG_GRAD_FLOW2, 0, nx, ny, nz, f, m2, col(6), ldout);
        const double *m3[7] = {col(3), col(4), col(5), fU, fV, fW, rP};
        run(dev, AVG_PROG_GRAD_FLOW3, p ? 1 : 0, nx, ny, nz, f, m3, col(44), ldout);
    }, TLAB_EINVAL);
}

int tlab_avg_ugradp(int nx, int ny, int nz, const double *u, const double *v, const double *w, const double *dpdx, const double *dpdy,
                    const double *dpdz, double *out) {
    (void)tlab_internal_deferred_flush();
    return catch_fail([&] {
        if (!u || !v || !w || !dpdx || !dpdy || !dpdz || !out) throw Fail(TLAB_EINVAL, "tlab_avg_ugradp: a null pointer");
        check_profiles("tlab_avg_ugradp", nx, ny, nz, ny);
        const double *f[6] = {u, v, w, dpdx, dpdy, dpdz};
        run(on_device("tlab_avg_ugradp", f, 6), AVG_PROG_UGRADP, 0, nx, ny, nz, f, nullptr, out, ny);
    }, TLAB_EINVAL);
}

int tlab_avg_gradients_scal(int nx, int ny, int nz, const double *const *grads, const double *s, const double *u, const double *v, const double *w,
                            const double *p, const double *fS, const double *fU, const double *fV, const double *fW, const double *rP,
                            const double *rS_y, const double *fS_y, double *out, int ldout) {
    (void)tlab_internal_deferred_flush();
    return catch_fail([&] {
        const char *who = "tlab_avg_gradients_scal";
        if (!grads || !grads[0] || !grads[1] || !grads[2] || !s || !u || !v || !w || !fS || !fU || !fV || !fW || !rS_y || !out ||
            (p == nullptr) != (rP == nullptr) || (p && !fS_y))
            throw Fail(TLAB_EINVAL, std::string(who) + ": a null pointer (p and rP may be NULL, together; fS_y is needed with p)");
        check_profiles(who, nx, ny, nz, ldout);
        const double *all[8] = {grads[0], grads[1], grads[2], s, u, v, w, p}, *f[8] = {grads[1], s, u, v, w, p, grads[0], grads[2]};
        const bool dev = on_device(who, all, p ? 8 : 7);
        auto col = [&](int c) { return out + (size_t)c * ldout; };
        run(dev, AVG_PROG_GRAD_SCAL1, 0, nx, ny, nz, grads, &rS_y, col(0), ldout);
        const double *m2[7] = {col(0), fS, fU, fV, fW, rP, fS_y};
        run(dev, AVG_PROG_GRAD_SCAL2, p ? 1 : 0, nx, ny, nz, f, m2, col(11), ldout);
    }, TLAB_EINVAL);
}

}  // extern "C"

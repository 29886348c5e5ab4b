// The monitors of the main loop on the single-domain driver: TIME_COURANT, MINMAX, FI_INVARIANT_P and DNS_BOUNDS_CONTROL's dilatation extremes
// (the kernels are in pointwise.hip and monitor.hip).
#include "../../include/tlab_amd.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "dns_state.hpp"
#include "monitor.hpp"

using namespace tlab;

// min / max of a device array through per-block partials reduced on the host (diagnostics: once per time step, not per substep)
static void minmax_impl(tlab_dns_t d, const double *a, const double *v, const double *w, int mode, int nx, int ny, int nz, double *mn, double *mx) {
    hipStream_t st = tlab_current_stream();
    const long long n = (long long)nx * ny * nz;
    const int nb = (int)std::min<long long>(1024, (n + 255) / 256);
    hk(launch_minmax_partial(a, v, w, d->od[0], d->od[1], d->od[2], mode, nx, ny, nz, d->koffset, d->nz_total > 1 ? 1 : 0, d->part, nb, st), "k_minmax_partial");
    std::vector<double> h((size_t)2 * nb);
    hk(hipMemcpyAsync(h.data(), d->part, (size_t)2 * nb * sizeof(double), hipMemcpyDeviceToHost, st), "hipMemcpy");
    hk(hipStreamSynchronize(st), "sync");
    *mn = *std::min_element(h.begin(), h.begin() + nb);
    *mx = *std::max_element(h.begin() + nb, h.end());
}

extern "C" {

int tlab_time_courant(tlab_dns_t d, double *const *q, double cfla, double cfld, double *pmax, double *dtime) {
    return catch_fail([&] {
        if (!d || !q || !pmax) throw Fail(TLAB_EINVAL, "tlab_time_courant: bad arguments");
        if (d->dx2i < 0.0) throw Fail(TLAB_EINVAL, "tlab_time_courant: the plans carry no Jacobian (tlab_fdm_plan_set_aux)");
        double mn, mx;
        minmax_impl(d, q[0], q[1], q[2], 1, d->nx, d->ny, d->nz, &mn, &mx);
        pmax[0] = mx;                                   // max of |u|/dx + |v|/dy + |w|/dz over the local box (time.f90:402-451)
        pmax[1] = d->schmidtfactor * d->dx2i;           // time.f90:466
        if (dtime && cfla > 0.0) *dtime = courant_dtime(cfla, cfld, pmax);      // (without a CFL number the caller's dtime stands)
    }, TLAB_EINVAL);
}

int tlab_fi_invariant_p(tlab_dns_t d, const double *u, const double *v, const double *w, double *result, double *tmp1) {
    return catch_fail([&] {
        if (!d || !u || !v || !w || !result || !tmp1) throw Fail(TLAB_EINVAL, "tlab_fi_invariant_p: bad arguments");
        const int nx = d->nx, ny = d->ny, nz = d->nz;
        const long long n = (long long)nx * ny * nz;
        hipStream_t st = tlab_current_stream();
        // result = -((du/dx + dv/dy) + dw/dz), fi_vectorcalculus.f90:130-136
        ok(tlab_opr_partial(1, d->g[0], TLAB_OPR_P1, nx, ny, nz, 0, u, result, nullptr), "OPR_Partial_X");
        ok(tlab_opr_partial(2, d->g[1], TLAB_OPR_P1, nx, ny, nz, 0, v, tmp1, nullptr), "OPR_Partial_Y");
        hk(launch_add1(result, tmp1, n, st), "add");
        ok(tlab_opr_partial(3, d->g[2], TLAB_OPR_P1, nx, ny, nz, 0, w, tmp1, nullptr), "OPR_Partial_Z");
        hk(launch_add1(result, tmp1, n, st), "add");
        hk(launch_negate(result, n, st), "negate");
    }, TLAB_EINVAL);
}

// FI_VORTICITY (mappings/fi_vorticity.f90:28-59): the six derivatives in the reference's order, kept in txc6, then one pass over them
int tlab_fi_vorticity(tlab_dns_t d, const double *u, const double *v, const double *w, double *result, double *const *txc6) {
    return catch_fail([&] {
        if (!d || !u || !v || !w || !result || !txc6) throw Fail(TLAB_EINVAL, "tlab_fi_vorticity: bad arguments");
        for (int i = 0; i < 6; ++i)
            if (!txc6[i]) throw Fail(TLAB_EINVAL, "tlab_fi_vorticity: a null txc array");
        const int nx = d->nx, ny = d->ny, nz = d->nz;
        const double *fld[6] = {v, u, u, w, w, v};      // v,x  u,y  u,z  w,x  w,y  v,z
        const int dir[6] = {1, 2, 3, 1, 2, 3};
        for (int i = 0; i < 6; ++i) ok(tlab_opr_partial(dir[i], d->g[dir[i] - 1], TLAB_OPR_P1, nx, ny, nz, 0, fld[i], txc6[i], nullptr), "OPR_Partial");
        hk(launch_vorticity_magnitude(txc6[0], txc6[1], txc6[2], txc6[3], txc6[4], txc6[5], result, (long long)nx * ny * nz, tlab_current_stream()),
           "k_vorticity_magnitude");
    }, TLAB_EINVAL);
}

// ... and the pass on its own, for arrays of either kind (classified like tlab_minmax_any; a mix is refused)
int tlab_vorticity_from_gradients(long long n, const double *vx, const double *uy, const double *uz, const double *wx, const double *wy,
                                  const double *vz, double *result) {
#pragma clang fp contract(off)      // the host loop keeps every operation as written, like the kernel
    (void)tlab_internal_deferred_flush();
    return catch_fail([&] {
        const char *who = "tlab_vorticity_from_gradients";
        const double *a[7] = {vx, uy, uz, wx, wy, vz, result};
        if (n < 1 || n > 0x7fffffffLL) throw Fail(TLAB_EINVAL, std::string(who) + ": n must be 1 to 2^31 - 1");
        int ndev = 0;
        for (const double *p : a) {
            if (!p) throw Fail(TLAB_EINVAL, std::string(who) + ": a null pointer");
            const int on = tlab_device_ready() ? tlab_pointer_on_device(p) : 0;
            if (on < 0) throw Fail(on, std::string(who) + ": " + tlab_last_error());
            ndev += on ? 1 : 0;
        }
        if (ndev != 0 && ndev != 7) throw Fail(TLAB_EINVAL, std::string(who) + ": host and device arrays in one call");
        if (ndev) hk(launch_vorticity_magnitude(vx, uy, uz, wx, wy, vz, result, n, tlab_current_stream()), "k_vorticity_magnitude");
        else
            for (long long i = 0; i < n; ++i)
                result[i] = ((vx[i] - uy[i]) * (vx[i] - uy[i]) + (uz[i] - wx[i]) * (uz[i] - wx[i])) + (wy[i] - vz[i]) * (wy[i] - vz[i]);
    }, TLAB_EINVAL);
}

// Section 3 of AVG_FLOW_XZ (statistics/avg_flow_xz.f90:976-986) in front of the gradient statistics, and with p the pressure block (:670-674) in
// front of that: the derivatives by the driver's plans, bcs = 0, into the reference's arrays (dudx .. dwdz = txc[0..8]; dp/dx, dp/dy, dp/dz in
// dwdx, dwdy, dwdz first)
int tlab_dns_avg_gradients_flow(tlab_dns_t d, double *const *q, const double *p, double *const *txc, const double *fU, const double *fV,
                                const double *fW, const double *rP, const double *rU_y, const double *rV_y, const double *rW_y, double *out,
                                int ldout) {
    return catch_fail([&] {
        const char *who = "tlab_dns_avg_gradients_flow";
        if (!d || !q || !txc || !fU || !fV || !fW || !rU_y || !rV_y || !rW_y || !out || (p == nullptr) != (rP == nullptr))
            throw Fail(TLAB_EINVAL, std::string(who) + ": a null pointer (p and rP may be NULL, together)");
        for (int i = 0; i < 3; ++i)
            if (!q[i]) throw Fail(TLAB_EINVAL, std::string(who) + ": a null velocity array");
        for (int i = 0; i < 9; ++i)
            if (!txc[i]) throw Fail(TLAB_EINVAL, std::string(who) + ": a null txc array");
        const int nx = d->nx, ny = d->ny, nz = d->nz;
        if (ldout < ny) throw Fail(TLAB_EINVAL, std::string(who) + ": the leading dimension of the profiles is smaller than ny");
        if (p) {
            for (int dir = 1; dir <= 3; ++dir) ok(tlab_opr_partial(dir, d->g[dir - 1], TLAB_OPR_P1, nx, ny, nz, 0, p, txc[5 + dir], nullptr), "OPR_Partial(p)");
            ok(tlab_avg_ugradp(nx, ny, nz, q[0], q[1], q[2], txc[6], txc[7], txc[8], out + (size_t)56 * ldout), "tlab_avg_ugradp");
        }
        for (int c = 0; c < 3; ++c)
            for (int dir = 1; dir <= 3; ++dir)
                ok(tlab_opr_partial(dir, d->g[dir - 1], TLAB_OPR_P1, nx, ny, nz, 0, q[c], txc[3 * c + dir - 1], nullptr), "OPR_Partial");
        ok(tlab_avg_gradients_flow(nx, ny, nz, txc, q[0], q[1], q[2], p, fU, fV, fW, rP, rU_y, rV_y, rW_y, out, ldout), "tlab_avg_gradients_flow");
    }, TLAB_EINVAL);
}

// ... and of one scalar (statistics/avg_scal_xz.f90:446-448, :602-604): dsdx, dsdy, dsdz = txc[0..2]
int tlab_dns_avg_gradients_scal(tlab_dns_t d, const double *s, double *const *q, const double *p, double *const *txc, const double *fS,
                                const double *fU, const double *fV, const double *fW, const double *rP, const double *rS_y, const double *fS_y,
                                double *out, int ldout) {
    return catch_fail([&] {
        const char *who = "tlab_dns_avg_gradients_scal";
        if (!d || !s || !q || !txc || !q[0] || !q[1] || !q[2] || !txc[0] || !txc[1] || !txc[2] || !out)
            throw Fail(TLAB_EINVAL, std::string(who) + ": a null pointer");
        const int nx = d->nx, ny = d->ny, nz = d->nz;
        for (int dir = 1; dir <= 3; ++dir) ok(tlab_opr_partial(dir, d->g[dir - 1], TLAB_OPR_P1, nx, ny, nz, 0, s, txc[dir - 1], nullptr), "OPR_Partial");
        ok(tlab_avg_gradients_scal(nx, ny, nz, txc, s, q[0], q[1], q[2], p, fS, fU, fV, fW, rP, rS_y, fS_y, out, ldout), "tlab_avg_gradients_scal");
    }, TLAB_EINVAL);
}

int tlab_minmax(tlab_dns_t d, const double *a, int nx, int ny, int nz, double *amn, double *amx) {
    return catch_fail([&] {
        if (!d || !a || !amn || !amx) throw Fail(TLAB_EINVAL, "tlab_minmax: bad arguments");
        minmax_impl(d, a, nullptr, nullptr, 0, nx, ny, nz, amn, amx);
    }, TLAB_EINVAL);
}

// DNS_BOUNDS_CONTROL (dns_local.f90:157-230), incompressible and anelastic: div(q) accumulated into txc[0] by the three P1 derivatives, then one
// reduction for min, max and their first locations.  Anelastic runs weight the velocities by rbackground first (:160-162, into txc[2..4]).
int tlab_dns_dilatation_extremes(tlab_dns_t d, double *const *q, double *const *txc, double *dil_min, double *dil_max, int *loc_min, int *loc_max) {
    return catch_fail([&] {
        if (!d || !q || !txc || !dil_min || !dil_max) throw Fail(TLAB_EINVAL, "tlab_dns_dilatation_extremes: bad arguments");
        if (d->stagger) throw Fail(TLAB_EUNSUPPORTED, "tlab_dns_dilatation_extremes: FI_INVARIANT_P_STAG (staggered pressure) is not built on the device");
        hipStream_t st = tlab_current_stream();      // (a recorded substep runs first: q is read below)
        follow_anelastic(d);
        const int nx = d->nx, ny = d->ny, nz = d->nz;
        const long long n = (long long)nx * ny * nz;
        const double *u = q[0], *v = q[1], *w = q[2];
        if (d->rb) {      // Thermo_Anelastic_WEIGHT_OUTPLACE(.., rbackground, q(1, i), txc(1, 2 + i))
            for (int i = 0; i < 3; ++i) hk(launch_weight_y(txc[2 + i], q[i], d->rb, nx, ny, n, 0, st), "k_weight_y");
            u = txc[2]; v = txc[3]; w = txc[4];
        }
        ok(tlab_opr_partial_add(1, d->g[0], nx, ny, nz, 0, u, nullptr, 0.0, txc[0], 0, txc[5], txc[6]), "OPR_Partial_X");
        ok(tlab_opr_partial_add(2, d->g[1], nx, ny, nz, 0, v, nullptr, 0.0, txc[0], 1, txc[5], txc[6]), "OPR_Partial_Y");
        ok(tlab_opr_partial_add(3, d->g[2], nx, ny, nz, 0, w, nullptr, 0.0, txc[0], 1, txc[5], txc[6]), "OPR_Partial_Z");
        long long imn = 0, imx = 0;
        hk(monitor_extremes(txc[0], nullptr, n, dil_min, dil_max, &imn, &imx, st), "k_extremes");
        auto loc = [&](long long e, int *ijk) {      // 1-based, k global (tlab_dns_set_slab)
            if (!ijk) return;
            ijk[0] = (int)(e % nx) + 1; ijk[1] = (int)((e / nx) % ny) + 1; ijk[2] = (int)(e / ((long long)nx * ny)) + 1 + d->koffset;
        };
        loc(imn, loc_min);
        loc(imx, loc_max);
    }, TLAB_EINVAL);
}

// the TIME_COURANT maximum of a box (nx, ny, nz) at global offsets (ioff, koff), with this driver's tables (the decomposed drivers' monitors)
int tlab_internal_dns_courant(tlab_dns_t d, const double *u, const double *v, const double *w, int nx, int ny, int nz, int ioff, int koff, double *pmax) {
    return catch_fail([&] {
        if (d->dx2i < 0.0) throw Fail(TLAB_EINVAL, "TIME_COURANT: the plans carry no Jacobian (tlab_fdm_plan_set_aux)");
        hipStream_t st = tlab_current_stream();
        hk(monitor_courant_max(u, v, w, d->od[0], d->od[1], d->od[2], nx, ny, nz, ioff, koff, d->nz_total > 1 ? 1 : 0, &pmax[0], st), "k_courant");
        pmax[1] = d->schmidtfactor * d->dx2i;
    }, TLAB_EINVAL);
}

// MINMAX (utils/minmax.f90:6), local part, of any device array: no driver needed
int tlab_device_minmax(const double *a, long long n, double *amn, double *amx) {
    return catch_fail([&] {
        if (!a || n < 1 || !amn || !amx) throw Fail(TLAB_EINVAL, "tlab_device_minmax: bad arguments");
        if (!tlab_device_ready()) throw Fail(TLAB_EHIP, "tlab_init has not been called (no CPU fallback exists)");
        hk(monitor_extremes(a, nullptr, n, amn, amx, nullptr, nullptr, tlab_current_stream()), "k_extremes");
    }, TLAB_EINVAL);
}

// ... of an array of either kind (the drop-in MINMAX): device memory takes the kernel, host memory the host loop of minmax.f90 -- a host array
// never reaches a kernel, a device array is never read by the host.  Without tlab_init no array is the library's: the host loop.
int tlab_minmax_any(const double *a, long long n, double *amn, double *amx) {
    if (!a || n < 1 || !amn || !amx) { tlab_set_error("tlab_minmax_any: bad arguments"); return TLAB_EINVAL; }
    const int on = tlab_device_ready() ? tlab_pointer_on_device(a) : 0;
    if (on < 0) return on;
    if (on) return tlab_device_minmax(a, n, amn, amx);
    double mn = a[0], mx = a[0];
    for (long long i = 1; i < n; ++i) { mn = std::min(mn, a[i]); mx = std::max(mx, a[i]); }
    *amn = mn; *amx = mx;
    return TLAB_OK;
}

}  // extern "C"

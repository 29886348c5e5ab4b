// The single-domain driver apart from its substep: creation and destruction, the tlab_dns_set_* entries, what the rest of the library asks the
// driver (tlab_internal_dns_*), and the launches of the buffer zones, the body forces, the diagnostic liquid and the scalar source, which the
// substep (rhs.cpp) shares with entry points of their own.
#include "../../include/tlab_amd.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <memory>
#include <string>
#include <vector>

#include "dns_state.hpp"
#include "int1_generic.hpp"

using namespace tlab;

long long tlab_internal_dns_points(tlab_dns_t d) { return d ? (long long)d->nx * d->ny * d->nz : 0; }
int tlab_internal_dns_nscal(tlab_dns_t d) { return d ? d->nscal : 0; }
tlab_poisson_plan_t tlab_internal_dns_poisson(tlab_dns_t d) { return d ? d->poisson : nullptr; }
int tlab_internal_dns_scal_arrays(tlab_dns_t d) { return d ? d->scal_arrays() : 0; }
bool tlab_internal_dns_has_bounds(tlab_dns_t d) { return d && d->bounds.any(); }
bool tlab_internal_dns_has_flow_zones(tlab_dns_t d) { return d && (d->buff[0][0].size > 0 || d->buff[0][1].size > 0); }
bool tlab_internal_dns_has_scal_zones(tlab_dns_t d) { return d && d->nscal > 0 && (d->buff[1][0].size > 0 || d->buff[1][1].size > 0); }
bool tlab_internal_dns_has_forces(tlab_dns_t d) { return d && d->force.any(); }
bool tlab_internal_check_bounds(const char *who, int nscal, int n, const int *active, const double *lo, const double *hi, std::vector<char> &on,
                                std::vector<double> &blo, std::vector<double> &bhi) {
    on.clear(); blo.clear(); bhi.clear();
    if (!active) return true;
    if (n < 0 || n > nscal || !lo || !hi) {
        tlab_set_error(std::string(who) + ": " + std::to_string(n) + " bounds for " + std::to_string(nscal) + " scalars, or NULL lo / hi");
        return false;
    }
    on.assign((size_t)nscal, 0);
    blo.assign((size_t)nscal, 0.0);
    bhi.assign((size_t)nscal, 0.0);
    bool any = false;
    for (int is = 0; is < n; ++is) {
        if (!active[is]) continue;
        if (std::isnan(lo[is]) || std::isnan(hi[is]) || lo[is] > hi[is]) {
            tlab_set_error(std::string(who) + ": scalar " + std::to_string(is + 1) + " has bounds [" + std::to_string(lo[is]) + ", " + std::to_string(hi[is]) +
                           "] (NaN, or min > max)");
            on.clear(); blo.clear(); bhi.clear();
            return false;
        }
        on[is] = 1; blo[is] = lo[is]; bhi[is] = hi[is];
        any = true;
    }
    if (!any) { on.clear(); blo.clear(); bhi.clear(); }      // nothing active: the kernels of a run without bounds
    return true;
}

void tlab_internal_dns_grid(tlab_dns_t d, tlab_dns_grid *out) {
    follow_anelastic(d);
    *out = {d->nx, d->ny, d->nz, {d->g[0], d->g[1], d->g[2]}, d->rb != nullptr, &d->particles};
}

namespace tlab {
void buffer_relax(tlab_dns *d, int group, double *const *a, double *const *h, hipStream_t st) {
    for (const tlab_dns::BufferBlock &b : d->buff[group]) {
        if (b.size == 0) continue;
        const long long zone = (long long)d->nx * b.size * d->nz;
        for (int f0 = 0; f0 < b.nf; f0 += 4)
            hk(launch_buffer_relax(std::min(4, b.nf - f0), h + f0, a + f0, b.ref + f0 * zone, b.tau + (long long)f0 * b.size, d->nx, d->ny, d->nz, b.offset,
                                   b.size, st), "buffer zone");
    }
}

void body_force(tlab_dns *d, double *const *q, double *const *s, double *const *hq, hipStream_t st) {
    hk(launch_body_force(d->force, hq, q, s, d->bprof, d->nx, d->ny, d->nz, st), "body force");
}

void diagnostic(tlab_dns *d, double *const *s, hipStream_t st) {
    if (d->mixture != TLAB_MIXT_AIRWATERLINEAR) return;
    const int ns = d->nscal;
    if (!s[ns] || !s[0] || (ns > 1 && !s[1])) throw Fail(TLAB_EINVAL, "FI_DIAGNOSTIC: null array (with a mixture s holds nscal + 1 arrays, the last the liquid)");
    hk(launch_airwater_linear(s[ns], s[0], ns > 1 ? s[1] : nullptr, ns, d->thermo_param[0], ns > 1 ? d->thermo_param[1] : 0.0, d->thermo_param[ns],
                              (long long)d->nx * d->ny * d->nz, st), "liquid");
}

void sources_scal(tlab_dns *d, double *const *s, double *const *hs, double *scr1, double *scr2, hipStream_t st) {
    if (!d->infrared_on()) return;
    if (d->rb) throw Fail(TLAB_EUNSUPPORTED, "[Infrared] in an anelastic run (Thermo_Anelastic_WEIGHT_INPLACE / _ADD of the source) is not built on the device");
    const int is = d->ir.scalar - 1;
    if (!s[d->nscal] || !hs[is] || !scr1 || !scr2) throw Fail(TLAB_EINVAL, "TLab_Sources_Scal: null array (liquid, tendency or scratch)");
    hk(launch_infrared_y(s[d->nscal], hs[is], scr1, scr2, d->ir.tab, d->ir.C, d->ir.kappa, d->ir.flux_top, d->ir.flux_bottom, d->nx, d->ny, d->nz, st),
       "infrared");
}
}  // namespace tlab

extern "C" {

// the wall-plane weights of a Neumann variant for the other drivers of the library (slab.cpp): 1 and (w = [2][K] device weights, K) when available
int tlab_internal_dns_neumann_weights(tlab_dns_t d, int ibc, const double **w, int *K) {
    try {
        if (!d || ibc < 1 || ibc > 3 || !neumann_weights(d, ibc)) return 0;
        *w = d->neuw[ibc].w;
        *K = d->neuw[ibc].K;
        return 1;
    } catch (...) {
        return 0;
    }
}

int tlab_dns_create(tlab_dns_t *out, tlab_fdm_plan_t gx, tlab_fdm_plan_t gy, tlab_fdm_plan_t gz, tlab_poisson_plan_t poisson,
                    int nx, int ny, int nz, int nscal, double visc, const double *schmidt) {
    return catch_fail([&] {
        if (!out || !gx || !gy || !gz || !poisson || nscal < 0 || (nscal > 0 && !schmidt) || visc <= 0.0)
            throw Fail(TLAB_EINVAL, "tlab_dns_create: bad arguments");
        if (!tlab_device_ready()) throw Fail(TLAB_EHIP, "tlab_init has not been called (no CPU fallback exists)");
        auto d = std::make_unique<tlab_dns>();
        d->g[0] = gx; d->g[1] = gy; d->g[2] = gz;
        d->poisson = poisson;
        d->nx = nx; d->ny = ny; d->nz = nz; d->nscal = nscal; d->visc = visc;
        d->stagger = tlab_fdm_plan_info(gx, 7) == 1 || (nz > 1 && tlab_fdm_plan_info(gz, 7) == 1);
        if (d->stagger && (tlab_fdm_plan_info(gx, 7) != 1 || (nz > 1 && tlab_fdm_plan_info(gz, 7) != 1)))
            throw Fail(TLAB_EINVAL, "staggering: both the x and the z plan need their interpolation tables (tlab_fdm_plan_set_stagger)");
        d->schmidt.assign(schmidt, schmidt + nscal);
        d->bcs.all_dirichlet(nscal);
        hk(hipMalloc((void **)&d->bcs_hb, (size_t)nx * nz * sizeof(double)), "hipMalloc");
        hk(hipMalloc((void **)&d->bcs_ht, (size_t)nx * nz * sizeof(double)), "hipMalloc");
        // TIME_INITIALIZE, tools/dns/time.f90:138-176
        d->nz_total = gz->t.n;
        double sf = 1.0;                                            // (prandtl = 1: incompressible)
        for (int is = 0; is < nscal; ++is) sf = std::max(sf, 1.0 / schmidt[is]);
        d->schmidtfactor = sf * visc;
        std::vector<double> o2[3];
        tlab_fdm_plan_t gg[3] = {gx, gy, gz};
        for (int ig = 0; ig < 3; ++ig) {
            const int m = gg[ig]->t.n;
            std::vector<double> o1(m);
            o2[ig].resize(m);
            const bool have_jac = (int)gg[ig]->t.jac.size() >= m;      // host-built plans carry it only after tlab_fdm_plan_set_aux
            if (!have_jac) d->dx2i = -1.0;
            for (int i = 0; i < m; ++i) { o1[i] = have_jac ? 1.0 / gg[ig]->t.jac[i] : 0.0; o2[ig][i] = o1[i] * o1[i]; }
            hk(hipMalloc((void **)&d->od[ig], (size_t)m * sizeof(double)), "hipMalloc");
            hk(hipMemcpy(d->od[ig], o1.data(), (size_t)m * sizeof(double), hipMemcpyHostToDevice), "hipMemcpy");
        }
        if (d->dx2i >= 0.0) {   // separable maximum of the sum = sum of the maxima over the directions with more than one point
            d->dx2i = 0.0;
            for (int ig = 0; ig < 3; ++ig)
                if (gg[ig]->t.n > 1) d->dx2i += *std::max_element(o2[ig].begin(), o2[ig].end());
        }
        hk(hipMalloc((void **)&d->part, (size_t)2 * 1024 * sizeof(double)), "hipMalloc");
        *out = d.release();
    }, TLAB_EINVAL);
}

int tlab_dns_destroy(tlab_dns_t d) {
    (void)tlab_internal_deferred_flush();
    // the operator state THIS driver switched on goes with it; one set through tlab_opr_burgers_set_anelastic (OPR_Burgers_AMD_Anelastic) or by
    // another driver since is not this driver's to clear
    if (d && d->anel_owner && d->rb) {
        const double *rb, *rib;
        unsigned long ver;
        (void)tlab_internal_anelastic_state(&rb, &rib, &ver);
        if (ver == d->anel_version) (void)tlab_opr_burgers_set_anelastic(0, nullptr, nullptr);
    }
    delete d;
    return TLAB_OK;
}

int tlab_dns_set_bcs(tlab_dns_t d, const int *flow_jmin, const int *flow_jmax, const int *scal_jmin, const int *scal_jmax) {
    (void)tlab_internal_deferred_flush();
    return catch_fail([&] {
        if (!d) throw Fail(TLAB_EINVAL, "tlab_dns_set_bcs: bad arguments");
        d->bcs.set("tlab_dns_set_bcs", d->nscal, flow_jmin, flow_jmax, scal_jmin, scal_jmax);
        // the wall-plane weights of the Neumann variants in use are built HERE (allocations, a synchronisation), not in the middle of the first substep
        for (int i = 0; i < 3; ++i)
            if (d->bcs.flow_variant(i)) (void)neumann_weights(d, d->bcs.flow_variant(i));
        for (int i = 0; i < d->nscal; ++i)
            if (d->bcs.scal_variant(i)) (void)neumann_weights(d, d->bcs.scal_variant(i));
    }, TLAB_EHIP);
}

// BcsScalJmin/Jmax%SfcType and %cpl of the scalars ([BoundaryConditions] Scalar<i>SfcTypeJmin/Jmax = static | linear, Scalar<i>CouplingJmin/Jmax;
// boundary_bcs.f90:76-87): 0 = DNS_SFC_STATIC, 1 = DNS_SFC_LINEAR.  Single-domain driver only (the plane average is an all-reduce in a decomposed run).
int tlab_dns_set_surface_bcs(tlab_dns_t d, const int *sfc_jmin, const int *sfc_jmax, const double *cpl_jmin, const double *cpl_jmax) {
    (void)tlab_internal_deferred_flush();
    if (!d || (d->nscal > 0 && (!sfc_jmin || !sfc_jmax || !cpl_jmin || !cpl_jmax))) {
        tlab_set_error("tlab_dns_set_surface_bcs: bad arguments");
        return TLAB_EINVAL;
    }
    return catch_fail([&] {
        for (int i = 0; i < d->nscal; ++i)
            if ((sfc_jmin[i] != 0 && sfc_jmin[i] != 1) || (sfc_jmax[i] != 0 && sfc_jmax[i] != 1)) throw Fail(TLAB_EINVAL, "SfcType: 0 static or 1 linear");
        d->sfc_jmin.assign(sfc_jmin, sfc_jmin + d->nscal); d->sfc_jmax.assign(sfc_jmax, sfc_jmax + d->nscal);
        d->cpl_jmin.assign(cpl_jmin, cpl_jmin + d->nscal); d->cpl_jmax.assign(cpl_jmax, cpl_jmax + d->nscal);
        d->sref_b.resize(d->nscal, nullptr); d->sref_t.resize(d->nscal, nullptr);
        const size_t pbytes = (size_t)d->nx * d->nz * sizeof(double);
        for (int i = 0; i < d->nscal; ++i) {
            if ((sfc_jmin[i] == 1 || sfc_jmax[i] == 1) && !d->sref_b[i]) {
                hk(hipMalloc((void **)&d->sref_b[i], pbytes), "hipMalloc");
                hk(hipMalloc((void **)&d->sref_t[i], pbytes), "hipMalloc");
            }
        }
        if (!d->sfc_avg) hk(hipMalloc((void **)&d->sfc_avg, sizeof(double)), "hipMalloc");
    }, TLAB_EINVAL);
}

// nse_eqns == DNS_EQNS_ANELASTIC (tools/dns/rhs_global_incompressible_1.f90:211-214, 275-277, 326-329; physics/opr_burgers.f90:128-183) with the
// background profiles the host's thermodynamics made: rbackground(1:ny), ribackground(1:ny) = 1 / rbackground (HOST pointers; NULL: incompressible)
int tlab_dns_set_anelastic(tlab_dns_t d, const double *rbackground, const double *ribackground) {
    (void)tlab_internal_deferred_flush();
    if (!d) return TLAB_EINVAL;
    return catch_fail([&] {
        if (!rbackground || !ribackground) ok(tlab_opr_burgers_set_anelastic(0, nullptr, nullptr), "tlab_opr_burgers_set_anelastic");
        else ok(tlab_opr_burgers_set_anelastic(d->ny, rbackground, ribackground), "tlab_opr_burgers_set_anelastic");
        follow_anelastic(d);
        d->anel_owner = d->rb != nullptr;
    }, TLAB_EINVAL);
}

// [PressureFilter] (operators/opr_filter.f90:46, 78; rhs_global_incompressible_1.f90:286-290): directional 1-D filters applied to p and dp/dy after
// the Poisson solve; NULL = DNS_FILTER_NONE in that direction; repeat may be NULL (1 each).  The filters are not owned.
int tlab_dns_set_pressure_filter(tlab_dns_t d, tlab_filter_t fx, tlab_filter_t fy, tlab_filter_t fz, const int *repeat) {
    (void)tlab_internal_deferred_flush();
    if (!d) return TLAB_EINVAL;
    d->pfilter[0] = fx; d->pfilter[1] = fy; d->pfilter[2] = fz;
    for (int i = 0; i < 3; ++i) d->pfilter_rep[i] = repeat ? repeat[i] : 1;
    return TLAB_OK;
}

// [Filter] (operators/opr_filter.f90:45, FilterDomain; tools/dns/dns_filter.f90): the directional filters of DNS_FILTER.  Not owned.  What
// tlab_dns_filter would refuse is refused here, so that a driver never holds a filter it cannot apply.
int tlab_dns_set_filter(tlab_dns_t d, tlab_filter_t fx, tlab_filter_t fy, tlab_filter_t fz, const int *repeat) {
    (void)tlab_internal_deferred_flush();
    return catch_fail([&] {
        if (!d) throw Fail(TLAB_EINVAL, "tlab_dns_set_filter: null handle");
        const tlab_filter_t f[3] = {fx, fy, fz};
        tlab_internal_filter_fields(d->nx, d->ny, d->nz, f, repeat, 0, nullptr, tlab_current_stream(), "tlab_dns_set_filter");      // (no field: the checks alone)
        for (int i = 0; i < 3; ++i) { d->dfilter[i] = f[i]; d->dfilter_rep[i] = repeat ? repeat[i] : 1; }
    }, TLAB_EINVAL);
}

// DNS_FILTER (tools/dns/dns_filter.f90:69-104) without its kin statistics: OPR_FILTER on q and the prognostic scalars, DNS_BOUNDS_LIMIT, FI_DIAGNOSTIC
int tlab_dns_filter(tlab_dns_t d, double *const *q, double *const *s) {
    (void)tlab_internal_deferred_flush();
    return guarded([&] {
        if (!d || !q || (d->scal_arrays() > 0 && !s)) throw Fail(TLAB_EINVAL, "tlab_dns_filter: bad arguments");
        std::vector<double *> u(q, q + 3);
        u.insert(u.end(), s, s + d->nscal);
        for (int is = 0; is < d->scal_arrays(); ++is)
            if (!s[is]) throw Fail(TLAB_EINVAL, "tlab_dns_filter: null array (with a mixture s holds nscal + 1 arrays, the last the liquid)");
        hipStream_t st = tlab_current_stream();
        tlab_internal_filter_fields(d->nx, d->ny, d->nz, d->dfilter, d->dfilter_rep, (int)u.size(), u.data(), st, "tlab_dns_filter");
        const long long n = (long long)d->nx * d->ny * d->nz;
        for (int is = 0; is < d->nscal; ++is)
            if (d->bounds.active(is)) hk(launch_clip(s[is], d->bounds.lo[is], d->bounds.hi[is], n, st), "clip");
        diagnostic(d, s, st);
    });
}

int tlab_dns_set_remove_divergence(tlab_dns_t d, int on) {
    (void)tlab_internal_deferred_flush();
    if (!d) return TLAB_EINVAL;
    d->remove_divergence = on != 0;
    return TLAB_OK;
}

int tlab_dns_set_slab(tlab_dns_t d, int koffset) {
    (void)tlab_internal_deferred_flush();
    if (!d || koffset < 0 || koffset + d->nz > d->nz_total) { tlab_set_error("tlab_dns_set_slab: bad offset"); return TLAB_EINVAL; }
    d->koffset = koffset;
    return TLAB_OK;
}

int tlab_dns_begin_step(tlab_dns_t d) {
    (void)tlab_internal_deferred_flush();
    if (!d) return TLAB_EINVAL;
    d->fresh = true;
    return TLAB_OK;
}

int tlab_dns_set_scalar_bounds(tlab_dns_t d, int n, const int *active, const double *lo, const double *hi) {
    return set_scalar_bounds("tlab_dns_set_scalar_bounds", d, n, active, lo, hi);
}

int tlab_dns_set_fusion(tlab_dns_t d, int on) {
    (void)tlab_internal_deferred_flush();
    if (!d) return TLAB_EINVAL;
    d->fuse = on != 0;
    return TLAB_OK;
}

// ---- [BufferZone] Type = relaxation (tools/dns/boundary_buffer.f90) ----
// INI_BLOCK :359-371 on the host, in the reference's operation order: dummy = 1 / L, then strength * ((dy) * dummy) ** sigma
int tlab_buffer_tau(int n, const double *nodes, int offset, int size, double strength, double sigma, int form, double *tau_out) {
    if (!nodes || !tau_out || n < 1 || offset < 0 || size < 2 || offset + size > n || (form != 1 && form != 2)) {
        tlab_set_error(size == 1 ? "tlab_buffer_tau: a zone of one plane has no length (the reference leaves tau unset there)"
                                 : "tlab_buffer_tau: bad arguments (0 <= offset, 2 <= size, offset + size <= n, form 1 = Jmin or 2 = Jmax)");
        return TLAB_EINVAL;
    }
    const double dummy = 1.0 / (nodes[offset + size - 1] - nodes[offset]);
    for (int jloc = 0; jloc < size; ++jloc) {
        const int j = offset + jloc;
        const double dy = form == 2 ? nodes[j] - nodes[offset] : nodes[offset + size - 1] - nodes[j];
        tau_out[jloc] = strength * std::pow(dy * dummy, sigma);
    }
    return TLAB_OK;
}

int tlab_dns_set_buffer_type(tlab_dns_t d, int type) {
    (void)tlab_internal_deferred_flush();
    return catch_fail([&] {
        if (!d) throw Fail(TLAB_EINVAL, "tlab_dns_set_buffer_type: null handle");
        if (type == TLAB_BUFFER_FILTER || type == TLAB_BUFFER_BOTH)
            throw Fail(TLAB_EUNSUPPORTED, "[BufferZone] Type = filter / both: the filter zones are not built on the device (relaxation only)");
        if (type != TLAB_BUFFER_NONE && type != TLAB_BUFFER_RELAX) throw Fail(TLAB_EINVAL, "tlab_dns_set_buffer_type: unknown type");
        if (type == TLAB_BUFFER_NONE)
            for (auto &g : d->buff)
                for (tlab_dns::BufferBlock &b : g) tlab_dns::free_block(b, true);
    }, TLAB_EINVAL);
}

int tlab_dns_set_buffer_zone(tlab_dns_t d, int end, int group, int size, int nfields, const double *tau, const double *ref) {
    (void)tlab_internal_deferred_flush();
    return catch_fail([&] {
        if (!d) throw Fail(TLAB_EINVAL, "tlab_dns_set_buffer_zone: null handle");
        if (end == TLAB_BUFFER_IMIN || end == TLAB_BUFFER_IMAX)
            throw Fail(TLAB_EUNSUPPORTED, "buffer zones at Imin / Imax: x is periodic in this library (they belong to spatially evolving runs)");
        if ((end != TLAB_BUFFER_JMIN && end != TLAB_BUFFER_JMAX) || (group != TLAB_BUFFER_FLOW && group != TLAB_BUFFER_SCAL))
            throw Fail(TLAB_EINVAL, "tlab_dns_set_buffer_zone: end = TLAB_BUFFER_JMIN / _JMAX, group = TLAB_BUFFER_FLOW / _SCAL");
        tlab_dns::BufferBlock &b = d->buff[group == TLAB_BUFFER_FLOW ? 0 : 1][end == TLAB_BUFFER_JMIN ? 0 : 1];
        tlab_dns::BufferBlock nb;
        if (size != 0 && tau) {
            const int want = group == TLAB_BUFFER_FLOW ? 3 : d->nscal;
            if (nfields != want || nfields < 1) throw Fail(TLAB_EINVAL, "tlab_dns_set_buffer_zone: nfields must be 3 (flow) or nscal (scalars)");
            if (size == 1) throw Fail(TLAB_EINVAL, "tlab_dns_set_buffer_zone: a zone of one plane (the reference leaves its tau unset)");
            if (size < 0 || size > d->ny) throw Fail(TLAB_EINVAL, "tlab_dns_set_buffer_zone: size must lie in 2 .. ny");
            if (!ref) throw Fail(TLAB_EINVAL, "tlab_dns_set_buffer_zone: ref is NULL");
            for (long long i = 0; i < (long long)size * nfields; ++i)
                if (std::isnan(tau[i])) throw Fail(TLAB_EINVAL, "tlab_dns_set_buffer_zone: NaN in tau");
            nb.size = size; nb.nf = nfields; nb.offset = end == TLAB_BUFFER_JMIN ? 0 : d->ny - size;
            const size_t tb = (size_t)size * nfields * sizeof(double), rb = (size_t)d->nx * size * d->nz * nfields * sizeof(double);
            try {
                hk(hipMalloc((void **)&nb.tau, tb), "hipMalloc");
                hk(hipMalloc((void **)&nb.ref, rb), "hipMalloc");
                hk(hipMemcpy(nb.tau, tau, tb, hipMemcpyHostToDevice), "hipMemcpy");
                hk(hipMemcpy(nb.ref, ref, rb, hipMemcpyHostToDevice), "hipMemcpy");
            } catch (...) {
                if (nb.tau) (void)hipFree(nb.tau);
                if (nb.ref) (void)hipFree(nb.ref);
                throw;
            }
        }
        tlab_dns::free_block(b, true);
        b = nb;
    }, TLAB_EINVAL);
}

int tlab_dns_buffer_relax_flow(tlab_dns_t d, double *const *q, double *const *hq) {
    return guarded([&] {
        if (!d || !q || !hq) throw Fail(TLAB_EINVAL, "tlab_dns_buffer_relax_flow: bad arguments");
        for (int i = 0; i < 3; ++i)
            if (!q[i] || !hq[i]) throw Fail(TLAB_EINVAL, "tlab_dns_buffer_relax_flow: null array");
        buffer_relax(d, 0, q, hq, tlab_current_stream());
    });
}

int tlab_dns_buffer_relax_scal(tlab_dns_t d, double *const *s, double *const *hs) {
    return guarded([&] {
        if (!d || (d->nscal > 0 && (!s || !hs))) throw Fail(TLAB_EINVAL, "tlab_dns_buffer_relax_scal: bad arguments");
        for (int i = 0; i < d->nscal; ++i)
            if (!s[i] || !hs[i]) throw Fail(TLAB_EINVAL, "tlab_dns_buffer_relax_scal: null array");
        buffer_relax(d, 1, s, hs, tlab_current_stream());
    });
}

// ---- [Rotation] and [BodyForce]: TLab_Sources_Flow (src/physics/tlab_sources.f90:36-92) ----
static bool all_finite(const double *v, int n) {
    for (int i = 0; i < n; ++i)
        if (!std::isfinite(v[i])) return false;
    return true;
}

int tlab_dns_set_coriolis(tlab_dns_t d, int type, const double *vector, const double *parameters) {
    (void)tlab_internal_deferred_flush();
    return catch_fail([&] {
        if (type != TLAB_COR_NONE && type != TLAB_COR_EXPLICIT && type != TLAB_COR_NORMALIZED) throw Fail(TLAB_EINVAL, "tlab_dns_set_coriolis: unknown type");
        tlab::BodyForce F;
        if (type != TLAB_COR_NONE) {
            if (!vector || !all_finite(vector, 3)) throw Fail(TLAB_EINVAL, "tlab_dns_set_coriolis: vector is NULL or holds NaN / infinite values");
            for (int i = 0; i < 3; ++i) F.f[i] = vector[i];
            F.cor = 1;
        }
        if (type == TLAB_COR_NORMALIZED) {
            if (!parameters || !all_finite(parameters, 2)) throw Fail(TLAB_EINVAL, "tlab_dns_set_coriolis: parameters is NULL or holds NaN / infinite values");
            if (vector[0] != 0.0 || vector[2] != 0.0)
                throw Fail(TLAB_EINVAL, "[Rotation] Type = normalized: only the vector (0, f2, 0) is allowed (the reference stops on an active y equation)");
            F.cor = 2;
            F.geo_u = std::cos(parameters[0]) * parameters[1];       // rotation.f90:127-128, on the host
            F.geo_w = -std::sin(parameters[0]) * parameters[1];
        }
        if (!d) throw Fail(TLAB_EINVAL, "tlab_dns_set_coriolis: null handle");
        d->force.cor = F.cor; d->force.geo_u = F.geo_u; d->force.geo_w = F.geo_w;
        for (int i = 0; i < 3; ++i) d->force.f[i] = F.f[i];
    }, TLAB_EINVAL);
}

int tlab_dns_set_buoyancy(tlab_dns_t d, int type, const double *vector, int nscalars, const double *parameters, int nparameters, int inb_scal_array,
                          const double *bbackground) {
    (void)tlab_internal_deferred_flush();
    return catch_fail([&] {
        if (type == TLAB_BOD_EXPLICIT)
            throw Fail(TLAB_EUNSUPPORTED, "[BodyForce] Type = explicit needs Thermo_Anelastic_BUOYANCY, which is not built on the device");
        if (type == TLAB_BOD_NORMALIZEDMEAN || type == TLAB_BOD_SUBTRACTMEAN)
            throw Fail(TLAB_EUNSUPPORTED, "[BodyForce] Type = normalizedmean / subtractmean need the plane means FI_DIAGNOSTIC refreshes every substep: not built on the device");
        if (type != TLAB_BOD_NONE && (type < TLAB_BOD_HOMOGENEOUS || type > TLAB_BOD_QUADRATIC)) throw Fail(TLAB_EINVAL, "tlab_dns_set_buoyancy: unknown type");
        tlab::BodyForce F;
        std::vector<double> prof;
        if (type != TLAB_BOD_NONE) {
            if (!vector || !all_finite(vector, 3)) throw Fail(TLAB_EINVAL, "tlab_dns_set_buoyancy: vector is NULL or holds NaN / infinite values");
            if (nparameters < 0 || nscalars < 0 || inb_scal_array < 0 || (nparameters > 0 && !parameters) || !all_finite(parameters, nparameters))
                throw Fail(TLAB_EINVAL, "tlab_dns_set_buoyancy: negative counts, parameters NULL, or NaN / infinite parameters");
            if (!d) throw Fail(TLAB_EINVAL, "tlab_dns_set_buoyancy: null handle");
            auto par = [&](int i) { return i < nparameters ? parameters[i] : 0.0; };      // (a key the ini file leaves out reads as zero)
            for (int i = 0; i < 3; ++i) F.g[i] = vector[i];
            const int ny = d->ny;
            std::vector<double> ref((size_t)ny, 0.0);
            if (bbackground) {
                if (!all_finite(bbackground, ny)) throw Fail(TLAB_EINVAL, "tlab_dns_set_buoyancy: NaN / infinite values in bbackground");
                ref.assign(bbackground, bbackground + ny);
            }
            prof.resize((size_t)ny);
            if (type != TLAB_BOD_HOMOGENEOUS && d->nscal == 0) throw Fail(TLAB_EINVAL, "[BodyForce] Type = linear / bilinear / quadratic on a driver without scalars");
            if (type == TLAB_BOD_HOMOGENEOUS) {
                F.bod = 1; F.c[0] = par(0);
            } else if (type == TLAB_BOD_LINEAR) {
                if (d->mixture == TLAB_MIXT_NONE && nscalars > d->nscal)
                    throw Fail(TLAB_EUNSUPPORTED, "[BodyForce] linear: the buoyancy reads scalar arrays beyond the prognostic scalars (diagnostic arrays are not held on the device)");
                if (nscalars > d->scal_arrays())
                    throw Fail(TLAB_EUNSUPPORTED, "[BodyForce] linear: the buoyancy reads scalar arrays beyond the liquid (inb_scal_array = nscal + 1)");
                const double c0 = par(inb_scal_array);
                if (nscalars >= 1 && nscalars <= 3) {      // gravity.f90:255-277
                    F.bod = 2; F.ns = nscalars;
                    for (int is = 0; is < nscalars; ++is) F.c[is] = par(is);
                    for (int j = 0; j < ny; ++j) prof[j] = ref[j] - c0;
                } else {                                    // :279-291
                    F.bod = 3;
                    for (int is = 0; is < nscalars; ++is) {
                        if (!(std::fabs(par(is)) > 1.0e-20)) continue;      // small_wp
                        if (F.ns == tlab::BODY_FORCE_MAX_SCAL) throw Fail(TLAB_EUNSUPPORTED, "[BodyForce] linear: more than 6 scalars with a non-zero factor");
                        F.c[F.ns] = par(is); F.sidx[F.ns] = is; ++F.ns;
                    }
                    for (int j = 0; j < ny; ++j) prof[j] = c0 - ref[j];
                }
            } else if (type == TLAB_BOD_BILINEAR) {
                if (d->nscal < 2) throw Fail(TLAB_EINVAL, "[BodyForce] Type = bilinear needs two scalars");
                F.bod = 4; F.ns = 2;
                for (int i = 0; i < 3; ++i) F.c[i] = par(i);
                prof = ref;
            } else {
                F.bod = 5; F.ns = 1;
                const double h = par(1) / 2.0;
                F.c[0] = -par(0) / (h * h);                  // :306
                F.c[1] = par(1);
                if (!std::isfinite(F.c[0])) throw Fail(TLAB_EINVAL, "[BodyForce] Type = quadratic: parameters(2) = 0");
                prof = ref;
            }
        }
        if (!d) throw Fail(TLAB_EINVAL, "tlab_dns_set_buoyancy: null handle");
        if (F.bod >= 2) {
            const size_t bytes = (size_t)d->ny * sizeof(double);
            if (!d->bprof) hk(hipMalloc((void **)&d->bprof, bytes), "hipMalloc");
            hk(hipStreamSynchronize(tlab_current_stream()), "sync");      // (a kernel that reads the old profile may still be in flight)
            hk(hipMemcpy(d->bprof, prof.data(), bytes, hipMemcpyHostToDevice), "hipMemcpy");
        }
        d->bback = F.bod >= 2 && bbackground && std::any_of(bbackground, bbackground + d->ny, [](double v) { return v != 0.0; });
        d->force.bod = F.bod; d->force.ns = F.ns;
        for (int i = 0; i < 3; ++i) d->force.g[i] = F.g[i];
        for (int i = 0; i < tlab::BODY_FORCE_MAX_SCAL; ++i) { d->force.c[i] = F.c[i]; d->force.sidx[i] = F.sidx[i]; }
    }, TLAB_EINVAL);
}

int tlab_dns_sources_flow(tlab_dns_t d, double *const *q, double *const *s, double *const *hq) {
    return guarded([&] {
        if (!d || !q || !hq || (d->nscal > 0 && !s)) throw Fail(TLAB_EINVAL, "tlab_dns_sources_flow: bad arguments");
        body_force(d, q, s, hq, tlab_current_stream());
    });
}

// ---- [Thermodynamics] Mixture and [Infrared]: FI_DIAGNOSTIC and TLab_Sources_Scal ----
int tlab_dns_set_mixture(tlab_dns_t d, int mixture, const double *thermo_param, int nparam) {
    (void)tlab_internal_deferred_flush();
    return catch_fail([&] {
        if (mixture != TLAB_MIXT_NONE && mixture != TLAB_MIXT_AIRWATERLINEAR)
            throw Fail(TLAB_EUNSUPPORTED, "tlab_dns_set_mixture: only AirWaterLinear (12) and none (0) are built on the device");
        if (!d) throw Fail(TLAB_EINVAL, "tlab_dns_set_mixture: null handle");
        if (mixture == TLAB_MIXT_NONE) {
            if (d->force.bod == 2 || d->force.bod == 3)
                for (int i = 0; i < d->force.ns; ++i)
                    if (d->force.sidx[i] >= d->nscal) throw Fail(TLAB_EINVAL, "tlab_dns_set_mixture: the buoyancy set on this driver reads the liquid; switch it off first");
            d->mixture = TLAB_MIXT_NONE;
            d->thermo_param.clear();
            d->ir.type = TLAB_IR_NONE;      // (the infrared term reads the liquid: it goes with the mixture)
            return;
        }
        if (d->nscal < 1) throw Fail(TLAB_EINVAL, "tlab_dns_set_mixture: AirWaterLinear on a driver without scalars");
        if (!thermo_param || nparam < d->nscal + 1) throw Fail(TLAB_EINVAL, "tlab_dns_set_mixture: thermo_param needs nscal + 1 values");
        if (!all_finite(thermo_param, nparam)) throw Fail(TLAB_EINVAL, "tlab_dns_set_mixture: NaN / infinite values in thermo_param");
        d->mixture = mixture;
        d->thermo_param.assign(thermo_param, thermo_param + nparam);
    }, TLAB_EINVAL);
}

int tlab_dns_diagnostic(tlab_dns_t d, double *const *s) {
    return guarded([&] {
        if (!d || (d->scal_arrays() > 0 && !s)) throw Fail(TLAB_EINVAL, "tlab_dns_diagnostic: bad arguments");
        diagnostic(d, s, tlab_current_stream());
    });
}

int tlab_dns_set_infrared(tlab_dns_t d, int type, int scalar, double kappa, double flux_top, double flux_bottom) {
    (void)tlab_internal_deferred_flush();
    return catch_fail([&] {
        if (type == 2 || type == 3)
            throw Fail(TLAB_EUNSUPPORTED, "[Infrared] gray and band types need a temperature (the reference derives one for anelastic runs only): not built on the device");
        if (type != TLAB_IR_NONE && type != TLAB_IR_GRAY_LIQUID) throw Fail(TLAB_EINVAL, "tlab_dns_set_infrared: unknown type");
        if (!d) throw Fail(TLAB_EINVAL, "tlab_dns_set_infrared: null handle");
        if (type == TLAB_IR_NONE) { d->ir.type = TLAB_IR_NONE; return; }
        if (!std::isfinite(kappa) || !std::isfinite(flux_top) || !std::isfinite(flux_bottom)) throw Fail(TLAB_EINVAL, "tlab_dns_set_infrared: NaN / infinite values");
        if (d->mixture == TLAB_MIXT_NONE) throw Fail(TLAB_EINVAL, "[Infrared] gray liquid needs a mixture with a liquid field (tlab_dns_set_mixture); the reference stops there");
        if (scalar < 1 || scalar > d->nscal) throw Fail(TLAB_EINVAL, "tlab_dns_set_infrared: the term acts on one of the scalars 1..nscal");
        follow_anelastic(d);
        if (d->rb) throw Fail(TLAB_EUNSUPPORTED, "[Infrared] in an anelastic run (Thermo_Anelastic_WEIGHT_INPLACE / _ADD of the source) is not built on the device");
        const tlab::DerTables &g = d->g[1]->t.der1;
        if (tlab::int1_generic_applies(g) || g.ndl != 3 || g.ndr != 5 || g.periodic)
            throw Fail(TLAB_EUNSUPPORTED, "[Infrared]: the first-order integral of this y plan is not the pentadiagonal system of CompactJacobian6");
        if (!tlab_device_ready()) throw Fail(TLAB_EHIP, "tlab_init has not been called (no CPU fallback exists)");
        if (!d->ir.tab) {
            std::vector<double> tab;
            tlab::InfraredCoef C;
            try {
                tlab::infrared_build_tables(g, tab, C);
            } catch (const std::exception &e) {
                throw Fail(TLAB_EUNSUPPORTED, std::string("[Infrared]: ") + e.what());
            }
            double *p = nullptr;
            hk(hipMalloc((void **)&p, tab.size() * sizeof(double)), "hipMalloc");
            if (hipMemcpy(p, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(p); throw Fail(TLAB_EHIP, "hipMemcpy"); }
            d->ir.tab = p;
            d->ir.C = C;
        }
        d->ir.type = type; d->ir.scalar = scalar; d->ir.kappa = kappa; d->ir.flux_top = flux_top; d->ir.flux_bottom = flux_bottom;
    }, TLAB_EINVAL);
}

int tlab_dns_sources_scal(tlab_dns_t d, double *const *s, double *const *hs, double *const *txc) {
    return guarded([&] {
        if (!d || !txc || (d->nscal > 0 && (!s || !hs))) throw Fail(TLAB_EINVAL, "tlab_dns_sources_scal: bad arguments");
        sources_scal(d, s, hs, txc[0], txc[1], tlab_current_stream());
    });
}

long long tlab_dns_info(tlab_dns_t d, int what) {
    if (!d) return -1;
    switch (what) {
    case 0: return d->nx;
    case 1: return d->ny;
    case 2: return d->nz;
    case 3: return d->nscal;
    case 4: return (long long)d->nx * d->ny * d->nz;
    case 5: return d->scal_arrays();
    default: return -1;
    }
}

}  // extern "C"

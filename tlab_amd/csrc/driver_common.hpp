// What the three drivers (rhs.cpp with dns_setup.cpp: one domain, slab.cpp: z-slabs, pencil.cpp: x/z pencils) and zslab.hip share around their physics: the state
// and argument checks that do not depend on the decomposition (the error type and the guards of their entry points: errors.hpp).  Header-only, host code.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <stdexcept>
#include <string>
#include <vector>

#include "errors.hpp"
#include "internal.hpp"

namespace tlab {

// n doubles (at least one) of device memory, zeroed by a blocking hipMemset or -- on_stream -- by hipMemsetAsync on the library's current stream
inline double *dalloc(size_t n, bool on_stream) {
    const size_t bytes = std::max<size_t>(n, 1) * sizeof(double);
    double *p = nullptr;
    hk(hipMalloc((void **)&p, bytes), "hipMalloc");
    hk(on_stream ? hipMemsetAsync(p, 0, bytes, tlab_current_stream()) : hipMemset(p, 0, bytes), "hipMemset");
    return p;
}

// [Control] ScalLimit: DNS_BOUNDS_LIMIT (dns_local.f90:67-90) after the update of every substep, s = min(max(s, lo), hi) for the active scalars
struct ScalarBounds {
    std::vector<char> on;      // per scalar; empty: no scalar is limited (the kernels of a run without bounds)
    std::vector<double> lo, hi;
    bool any() const { return !on.empty(); }
    bool active(int is) const { return !on.empty() && on[is]; }
    // false (nothing changed, the reason in tlab_last_error()): see tlab_internal_check_bounds
    bool set(const char *who, int nscal, int n, const int *active_, const double *lo_, const double *hi_) {
        ScalarBounds b;
        if (!tlab_internal_check_bounds(who, nscal, n, active_, lo_, hi_, b.on, b.lo, b.hi)) return false;
        *this = std::move(b);
        return true;
    }
};
// tlab_*_set_scalar_bounds of a driver D with members nscal and bounds
template <class D>
int set_scalar_bounds(const char *who, D *d, int n, const int *active, const double *lo, const double *hi) {
    (void)tlab_internal_deferred_flush();
    if (!d) { tlab_set_error(std::string(who) + ": null handle"); return TLAB_EINVAL; }
    return d->bounds.set(who, d->nscal, n, active, lo, hi) ? TLAB_OK : TLAB_EINVAL;
}

// What the tail of ONE Runge-Kutta substep does beyond the RHS (TIME_SUBSTEP_INCOMPRESSIBLE_EXPLICIT, time.f90:559-664), handed as a value to the substep
// entry of each driver (internal.hpp): the public entries pass the driver's own settings, {kco, scale, &d->bounds, true, true, true}, the deferred tail what
// its record holds.  The RHS on its own is a call without a tail (a null pointer inside the drivers): no update, no scalar zones, no forces, no scalar sources.
struct SubstepTail {
    double kco;                       // hq, hs *= kco after the update ...
    int scale;                        // ... unless 0
    const ScalarBounds *bounds;       // DNS_BOUNDS_LIMIT after the update; null or empty: none
    bool scal_zones;                  // BOUNDARY_BUFFER_RELAX_SCAL: the scalar buffer blocks the driver holds act
    bool forces;                      // TLab_Sources_Flow: the body forces the driver holds act
    bool scal_sources = false;        // TLab_Sources_Scal: the infrared term the single-domain driver holds acts (no record of the deferred tail carries it)
    bool clips(int is) const { return bounds && bounds->active(is); }
};

// BcsFlowJmin/Jmax%type of u, v, w and BcsScalJmin/Jmax%type of the scalars (TLAB_DNS_BCS_*)
struct WallBcs {
    int flow_jmin[3] = {TLAB_DNS_BCS_DIRICHLET, TLAB_DNS_BCS_DIRICHLET, TLAB_DNS_BCS_DIRICHLET};
    int flow_jmax[3] = {TLAB_DNS_BCS_DIRICHLET, TLAB_DNS_BCS_DIRICHLET, TLAB_DNS_BCS_DIRICHLET};
    std::vector<int> scal_jmin, scal_jmax;
    void all_dirichlet(int nscal) {
        scal_jmin.assign(nscal, TLAB_DNS_BCS_DIRICHLET);
        scal_jmax.assign(nscal, TLAB_DNS_BCS_DIRICHLET);
    }
    // the Neumann variant of a field as BOUNDARY_BCS_NEUMANN_Y and the kernels take it: 0 none, 1 jmin, 2 jmax, 3 both (the other side Dirichlet)
    static int variant(int tmin, int tmax) { return (tmin == TLAB_DNS_BCS_NEUMANN ? 1 : 0) + (tmax == TLAB_DNS_BCS_NEUMANN ? 2 : 0); }
    int flow_variant(int i) const { return variant(flow_jmin[i], flow_jmax[i]); }
    int scal_variant(int is) const { return variant(scal_jmin[is], scal_jmax[is]); }
    // every wall of every velocity component is Dirichlet (no-slip)
    bool flow_dirichlet() const { return flow_variant(0) == 0 && flow_variant(1) == 0 && flow_variant(2) == 0; }
    // tlab_*_set_bcs (who = the entry point): throws, and leaves the types as they were, unless every type is valid
    void set(const std::string &who, int nscal, const int *fmin, const int *fmax, const int *smin, const int *smax) {
        if (!fmin || !fmax || (nscal > 0 && (!smin || !smax))) throw Fail(TLAB_EINVAL, who + ": bad arguments");
        auto valid = [](int t) { return t == TLAB_DNS_BCS_DIRICHLET || t == TLAB_DNS_BCS_NEUMANN; };
        for (int i = 0; i < 3; ++i)
            if (!valid(fmin[i]) || !valid(fmax[i])) throw Fail(TLAB_EINVAL, who + ": type must be DNS_BCS_DIRICHLET or DNS_BCS_NEUMANN");
        for (int i = 0; i < nscal; ++i)
            if (!valid(smin[i]) || !valid(smax[i])) throw Fail(TLAB_EINVAL, who + ": type must be DNS_BCS_DIRICHLET or DNS_BCS_NEUMANN");
        if (fmin[1] != TLAB_DNS_BCS_DIRICHLET || fmax[1] != TLAB_DNS_BCS_DIRICHLET)
            throw Fail(TLAB_EUNSUPPORTED, who + ": the wall-normal velocity must be Dirichlet (impermeable walls; the pressure BCs assume v = 0)");
        for (int i = 0; i < 3; ++i) { flow_jmin[i] = fmin[i]; flow_jmax[i] = fmax[i]; }
        for (int i = 0; i < nscal; ++i) { scal_jmin[i] = smin[i]; scal_jmax[i] = smax[i]; }
    }
};

// tlab_*_bind of the decomposed drivers: the module arrays of one local rank R (members q, s, hq, hs, txc, bound); no entry may be null (the
// first kernel would dereference it)
template <class R>
void bind_arrays(const std::string &who, int nscal, R &rank, double *const *q, double *const *s, double *const *hq, double *const *hs,
                 double *const *txc) {
    if (!q || !hq || !txc || (nscal > 0 && (!s || !hs))) throw Fail(TLAB_EINVAL, who + ": bad arguments");
    rank.q.assign(q, q + 3); rank.hq.assign(hq, hq + 3); rank.txc.assign(txc, txc + 9);
    rank.s.assign(s, s + nscal); rank.hs.assign(hs, hs + nscal);
    for (const std::vector<double *> *v : {&rank.q, &rank.s, &rank.hq, &rank.hs, &rank.txc})
        for (double *p : *v)
            if (!p) throw Fail(TLAB_EINVAL, who + ": null array");
    rank.bound = true;
}
// tlab_internal_{slab,pencil}_bound of a driver D with members rk (its local ranks), nscal, n and bounds
template <class D>
bool bound_fields(D *d, tlab_bound_fields *out) {
    if (!d || d->rk.size() != 1 || !d->rk[0].bound) return false;
    *out = {d->rk[0].q.data(), d->rk[0].s.data(), d->rk[0].hq.data(), d->rk[0].hs.data(), d->nscal, d->n, d->bounds.any()};
    return true;
}

// tlab_{slab,pencil}_dns_set_coriolis / _set_buoyancy of a decomposed driver D: y is never split, so the forces of a local rank live in its
// single-domain handle (handle(d, R), made on first use) and every one takes the same setting -- set(h) is the single-domain entry `what` on h
template <class D, class H, class F>
int set_on_ranks(D *d, H handle, const char *what, F set) {
    (void)tlab_internal_deferred_flush();
    return catch_fail([&] {
        if (!d) ok(set(nullptr), what);      // (the argument checks come first, as there)
        for (auto &R : d->rk) ok(set(handle(d, R)), what);
    }, TLAB_EINVAL);
}

// time.f90:523-538, explicit RK: the smaller of the advective and the diffusive limit of pmax (TIME_COURANT); 0 without a CFL number
inline double courant_dtime(double cfla, double cfld, const double *pmax) {
    const double dtc = pmax[0] > 0.0 ? cfla / pmax[0] : 1.0e300, dtd = pmax[1] > 0.0 ? cfld / pmax[1] : 1.0e300;
    return cfla > 0.0 ? std::min(dtc, dtd) : 0.0;
}

}  // namespace tlab

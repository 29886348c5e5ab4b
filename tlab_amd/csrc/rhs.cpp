// RHS_GLOBAL_INCOMPRESSIBLE_1 (tools/dns/rhs_global_incompressible_1.f90:15-405) and the explicit low-storage
// Runge-Kutta substep around it (TIME_SUBSTEP_INCOMPRESSIBLE_EXPLICIT, tools/dns/time.f90:559-664, and the scaling
// of the tendencies, :261-298), orchestrating the device operators so that no field leaves HBM during a substep.
// Same operator sequence, same scratch roles (tmp1..tmp9 = txc(:,1:9)) as the reference.
// This file is the substep and nothing else: the route (which launches a configuration makes, decided once), the stages that make them, the
// three entry points, and the one other route through the same stages, which stops at the pressure (FI_PRESSURE_BOUSSINESQ: pressure_boussinesq,
// tlab_dns_pressure).  The driver's state is in dns_state.hpp; its creation and settings in dns_setup.cpp.
#include "../../include/tlab_amd.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <string>
#include <vector>

#include "dns_state.hpp"

using namespace tlab;

// The wall value BOUNDARY_BCS_NEUMANN_Y (boundary_bcs.f90:368-473) gives a finished tendency h is a LINEAR functional of the y line:
// c0 h(2) + c1 h(3) + c2 h(4) + c3 (D_N h)(2) with D_N the first derivative under the Neumann variant of the system.  Its weights are found once per
// plan and variant by sending the unit vectors through the library's own routine (an ny x ny x 1 box holding the identity), and they decay like the
// coupling of the compact system (0.38^j): K = the rows beyond which they are below 1e-22 of the largest.  The wall planes of a field then cost a
// weighted sum over 2 K rows instead of a derivative pass over the field; and for u (w), whose finished tendency is hq - dp/dx (dp/dz), the sum
// commutes with the x (z) derivative: wall value = sum_j w_j hq(j) - d/dx [sum_j w_j p(j)] -- one derivative of a PLANE.
// (K <= ny always: on short lines the two sums overlap, which is as exact as the full line.)  Returns false where the weights are not finite.
bool tlab::neumann_weights(tlab_dns *d, int ibc) {
    tlab_dns::NeuW &W = d->neuw[ibc];
    if (W.tried) return W.w != nullptr;
    W.tried = true;
    const int ny = d->ny;
    const size_t N = (size_t)ny * ny;
    double *h = nullptr, *tmp = nullptr, *hb = nullptr, *ht = nullptr;
    auto release = [&] { for (double *p : {h, tmp, hb, ht}) if (p) (void)hipFree(p); };
    try {
        hk(hipMalloc((void **)&h, N * sizeof(double)), "hipMalloc");
        hk(hipMalloc((void **)&tmp, (N + 2 * (size_t)ny) * sizeof(double)), "hipMalloc");
        hk(hipMalloc((void **)&hb, (size_t)ny * sizeof(double)), "hipMalloc");
        hk(hipMalloc((void **)&ht, (size_t)ny * sizeof(double)), "hipMalloc");
        std::vector<double> id(N, 0.0);
        for (int j = 0; j < ny; ++j) id[(size_t)j * ny + j] = 1.0;       // column ix = j carries the unit vector e_j along y: h(ix, j) = delta
        hk(hipMemcpy(h, id.data(), N * sizeof(double), hipMemcpyHostToDevice), "hipMemcpy");
        hk(hipMemset(hb, 0, (size_t)ny * sizeof(double)), "hipMemset");
        hk(hipMemset(ht, 0, (size_t)ny * sizeof(double)), "hipMemset");
        // the copies above ran on the NULL stream, the routine below runs on the caller's stream (tlab_set_stream), which may be non-blocking: order them
        hk(hipDeviceSynchronize(), "hipDeviceSynchronize");
        ok(tlab_boundary_bcs_neumann_y(d->g[1], ibc, ny, ny, 1, h, hb, ht, tmp), "BOUNDARY_BCS_NEUMANN_Y (weights)");
        hk(hipStreamSynchronize(tlab_current_stream()), "sync");
        std::vector<double> wb(ny), wt(ny);
        hk(hipMemcpy(wb.data(), hb, (size_t)ny * sizeof(double), hipMemcpyDeviceToHost), "hipMemcpy");
        hk(hipMemcpy(wt.data(), ht, (size_t)ny * sizeof(double), hipMemcpyDeviceToHost), "hipMemcpy");
        release();
        h = tmp = hb = ht = nullptr;
        double mb = 0.0, mt = 0.0;
        for (int j = 0; j < ny; ++j) { mb = std::max(mb, std::fabs(wb[j])); mt = std::max(mt, std::fabs(wt[j])); }
        int K = 1;
        for (int j = 0; j < ny; ++j) {
            if ((ibc & 1) && std::fabs(wb[j]) > 1.0e-22 * mb) K = std::max(K, j + 1);
            if ((ibc & 2) && std::fabs(wt[ny - 1 - j]) > 1.0e-22 * mt) K = std::max(K, j + 1);
        }
        for (int j = 0; j < ny; ++j)
            if (!std::isfinite(wb[j]) || !std::isfinite(wt[j])) return false;
        if (((ibc & 1) && mb == 0.0) || ((ibc & 2) && mt == 0.0)) return false;       // weights that are all zero are never cached (the derivative pass serves then)
        // One Neumann wall only: the functional also sees the value on the OPPOSITE (Dirichlet) wall row through the biased closure there, with a weight
        // ~0.38^ny -- and the callers take their sums over tendencies whose Dirichlet wall row is already zeroed.  On lines so short that this weight
        // survives the cut (K reaches the other wall; measured 4.7e-10 at ny = 24) the route is not exact: the derivative pass serves.
        if (ibc != 3 && K >= ny) return false;
        std::vector<double> w((size_t)2 * K, 0.0);
        for (int j = 0; j < K; ++j) { w[j] = (ibc & 1) ? wb[j] : 0.0; w[K + j] = (ibc & 2) ? wt[ny - 1 - j] : 0.0; }
        hk(hipMalloc((void **)&W.w, w.size() * sizeof(double)), "hipMalloc");
        hk(hipMemcpy(W.w, w.data(), w.size() * sizeof(double), hipMemcpyHostToDevice), "hipMemcpy");
        W.K = K;
        return true;
    } catch (...) {
        release();
        throw;
    }
}

// The anelastic state lives with the operators (tlab_opr_burgers_set_anelastic = the module variables of OPR_Burgers_Initialize); the driver's density
// weights follow it, whichever entry point set it (tlab_dns_set_anelastic, tlab_opr_burgers_set_anelastic, Fortran OPR_Burgers_AMD_Anelastic), so the
// Burgers operators and the pressure step can never disagree about the equations being solved.
void tlab::follow_anelastic(tlab_dns *d) {
    const double *rb, *rib;
    unsigned long ver;
    const int ny = tlab_internal_anelastic_state(&rb, &rib, &ver);
    if (ver == d->anel_version) return;
    if (d->rb) { (void)hipFree(d->rb); d->rb = nullptr; }
    if (d->rib) { (void)hipFree(d->rib); d->rib = nullptr; }
    d->rb_wall[0] = d->rb_wall[1] = 1.0;
    if (ny > 0) {
        if (ny != d->ny) throw Fail(TLAB_EINVAL, "the anelastic profiles of the operators (tlab_opr_burgers_set_anelastic) have another ny than this driver");
        const size_t bytes = (size_t)ny * sizeof(double);
        hk(hipMalloc((void **)&d->rb, bytes), "hipMalloc");
        hk(hipMalloc((void **)&d->rib, bytes), "hipMalloc");
        hk(hipMemcpy(d->rb, rb, bytes, hipMemcpyHostToDevice), "hipMemcpy");
        hk(hipMemcpy(d->rib, rib, bytes, hipMemcpyHostToDevice), "hipMemcpy");
        d->rb_wall[0] = rb[0];
        d->rb_wall[1] = rb[ny - 1];
    }
    d->anel_version = ver;
}

namespace {
const int B0 = 0;      // bcs = 0: biased, non-zero (:67)

// Which launches a substep makes.  Every decision is taken ONCE, by decide_route below, before the first Burgers launch; the stages read it and
// decide nothing themselves (what a stage still tests at run time is whether a fused launch it was promised took place: an internal error if not).
// tail: the substep's SubstepTail, NULL in the RHS on its own.
struct Route {
    // ---- walls ----
    int ibc_q[3];                 // the Neumann variant of u, v, w (WallBcs::variant: 0 none, 1 jmin, 2 jmax, 3 both) ...
    std::vector<int> ibc_s;       // ... and of the scalars
    bool any_q;                   // a velocity component with a Neumann wall: its planes need the finished tendency first
    bool p_only;                  // the route stops at the pressure (PressureOnly below): no scalar equation, no dp/dy, nothing after the solve
    bool walls_dirichlet;         // no velocity wall is Neumann (a Neumann wall of any component sends all three through the unfused subtraction)
    bool any_surface;             // a scalar with the dynamic surface model: its wall planes are not zero, and it keeps planes of its own
    // ---- the equations: every fused form assumes the plain operators; anelastic runs, the staggered pressure grid
    // (rhs_global_incompressible_1.f90:216-226, 266-273, 307-317) and runs with [Dealiasing] take the literal sequence ----
    bool anel, stag, literal;
    bool pfilter;                 // a [PressureFilter] is set in some direction (:286-290)
    // ---- terms beside the Burgers sums ----
    // TLab_Sources_Flow runs before the RHS in the substep (time.f90:610-612), never in the RHS on its own
    bool forces;
    // ... and so does TLab_Sources_Scal (:611): the launch goes where hs holds a valid partial sum and the scalars are not finished yet, which is the
    // slot of the body forces on every route; tmp8, tmp9 are free there (the literal Burgers sums are done, the pressure step has not begun)
    bool scal_src;
    bool zone_flow, zone_scal;    // buffer zones act on the flow; on the scalars (the substep only)
    // ---- Burgers ----
    // Fused path: one launch per direction serves all equations (they share the advecting velocity of that direction), four fields per
    // launch.  The terms of an equation are then added in the order x, y, z instead of the reference's {1,2,3},{2,1,3},{3,1,2}: rounding only.
    // (the Burgers launches themselves only care about [Dealiasing]: the anelastic diffusion weight is inside the fused kernels where
    // tlab_internal_burgers_fusable says so, and the staggered pressure grid does not touch them; the epilogues are incompressible forms)
    bool batched;
    bool acc_direct;              // per-equation sums: a launch adds to the tendency itself where the fast kernels apply (else temp + k_add3)
    // The scalars have no pressure term: with Dirichlet walls their Runge-Kutta update (s += dte hs, hs *= kco; time.f90:645-664, :272-297) can
    // ride on the LAST Burgers launch that adds to hs, if that launch is the x one (the wave-per-line kernel has the registers for it; the
    // y/z tile kernels do not, measured).  The directions then run z, y, x instead of x, y, z: the terms are summed in another order, rounding only.
    // (TLAB_SCALAR_FINISH=0, read once per process, keeps x, y, z.)  x_last: the x launch runs last; finish_scal: and finishes the scalars.
    bool x_last, finish_scal;
    // Neumann scalars can ride too where the fused Neumann tail applies: the epilogue finishes their interior with zero wall tendencies, and the
    // wall planes follow from weighted sums over the stored tendencies next to the walls (neumann_weights; k_wall_fix) instead of a derivative pass
    // over the field (TLAB_NEUMANN_PLANES=0: that pass, k_rtile<P1+neumann final>)
    bool scal_neumann_planes;
    // Scalars under a buffer zone: the reference relaxes hs AFTER its wall BCs and BEFORE the update (time.f90:628-630).
    //  - Dirichlet scalars that the x Burgers epilogue finishes (zone_epi): the zone term joins hs in the mid-sequence zone launch, so the epilogue
    //    finishes every interior plane with it (summed in another order: rounding only).  The epilogue writes zero wall tendencies and leaves s on
    //    the wall planes as it was (clipped, which a field that came out of the last substep's clip already is): the wall planes inside a zone
    //    are redone by the plane form of the zone kernel, h = 0 - tau (s - ref), s += dte h, bounds, h *= kco.  Zone bytes only.
    //    (A pressure filter does not change this: the scalars never see the pressure.)
    //  - every other route (Neumann walls, whose wall value is a functional of the tendency WITHOUT the zone term; the surface model; the literal
    //    sequence): the literal order as passes of their own at the end -- wall planes, zone launch, k_rk_update (zone_tail).
    // The flow stays on the fused route either way.
    bool zone_epi, zone_tail;
    // Likewise the x term of the pressure forcing, d/dx (hq1 + u/dte) (:197-230): when the x Burgers launch runs last it holds the finished
    // tendency of u in registers, line by line, and differentiates it on the spot instead of a separate launch re-reading hq1 and u.
    bool div_in_burgers;
    // ... and the y and z terms, d/dy (hq2 + v/dte) and d/dz (hq3 + w/dte): each component gets the term of its OWN direction last, in a launch of
    // its own whose workgroups hold the finished tendency line by line and differentiate it on the spot (k_htile<BURGERS+div>).  Order of the
    // launches: z (all but w), y (all but v), x (all: finishes u, the scalars, writes the x term), y (v: adds the y term), z (w: adds the z term).
    // Against the three four-field launches + two forcing passes this saves the re-read of hq2, v, hq3, w (four passes of the eight).
    bool div_all;
    // ---- pressure ----
    bool fused_div;               // the three terms of the forcing as fused derivative launches that add into tmp1 (where the Burgers launches left any)
    // Neumann walls somewhere (free-slip u, w; Neumann scalars) and the fast kernels: the tail then runs per field -- gradient subtracted in its own
    // launch, BOUNDARY_BCS_NEUMANN_Y + final update in ONE launch along y (tlab_internal_neumann_final) -- and v, always Dirichlet, is finished by the solver
    bool neu_fast;
    // ... with the wall tendencies of u (w) from weighted sums over the rows next to the walls where the weights of its variant exist
    // (TLAB_NEUMANN_PLANES=0, read at every route: A/B in one process, keeps the derivative pass along y)
    bool flow_planes[3];
    // pressure in tmp1, Oy derivative in tmp3 (:284).  With Dirichlet walls for v and the RK update folded in, the last inverse transform of the
    // solver finishes the v equation itself (hq2 -= dp/dy; wall planes; v += dte hq2; hq2 *= kco) and tmp3 is not written
    bool v_final;
    // ---- pressure gradient (:319-320) ----
    // With Dirichlet walls and the RK update folded in (tail), the x- and z-gradient kernels finish u and w themselves: hq -= dp/dx; wall planes;
    // q += dte hq; hq *= kco (no gradient array is written or re-read)
    bool grad_final;
    // the gradient launches subtract themselves from the tendencies where the fused kernels apply (hq -= dp/dx: the same difference k_sub3 forms
    // from a stored gradient, two passes per component less); this is the tail of the RHS-only entry, i.e. of an unpatched Fortran host
    bool grad_sub;
    // Thermo_Anelastic_WEIGHT_SUBTRACT(.., ribackground, tmp2 | tmp3 | tmp4, hq(:,1) | hq(:,2) | hq(:,3))  (:326-329): a pass of its own, or -- for a
    // component with Dirichlet walls whose Runge-Kutta update follows (gw_defer) -- the operand of that update (k_final_update with gw)
    bool gw_defer[3];
};

// What a call that stops at the pressure (FI_PRESSURE_BOUSSINESQ, pressure_boussinesq below) asks of a route: the three momentum equations alone, no
// buffer zones (the reference's routine has none), and the body forces whether or not a tail is there.  NULL: the substep, or the RHS on its own.
struct PressureOnly { bool forces; };

// The one side effect: neumann_weights builds and caches the weights of a variant on first use (allocations, launches, a synchronisation; it may
// throw).  tlab_dns_set_bcs has built those of the variants in use, so inside a substep the call is a lookup.
Route decide_route(tlab_dns *d, const SubstepTail *tail, const PressureOnly *po = nullptr) {
    static const bool finish_off = [] { const char *e = getenv("TLAB_SCALAR_FINISH"); return e && atoi(e) == 0; }();
    const char *npe = getenv("TLAB_NEUMANN_PLANES");
    const bool neu_planes = !(npe && atoi(npe) == 0);
    const int nx = d->nx, ny = d->ny, nz = d->nz, ns = po ? 0 : d->nscal;
    tlab_fdm_plan_t gx = d->g[0], gy = d->g[1], gz = d->g[2];
    Route r;
    r.p_only = po != nullptr;
    bool scal_neu = false;
    r.any_q = r.any_surface = false;
    for (int iq = 0; iq < 3; ++iq) r.any_q = (r.ibc_q[iq] = d->bcs.flow_variant(iq)) != 0 || r.any_q;
    for (int is = 0; is < ns; ++is) {
        r.ibc_s.push_back(d->bcs.scal_variant(is));
        scal_neu = scal_neu || r.ibc_s[is] != 0;
        r.any_surface = r.any_surface || d->surface(is);
    }
    r.walls_dirichlet = d->bcs.flow_dirichlet();
    const bool dealias = tlab_internal_dealiasing();
    r.anel = d->rb != nullptr;
    r.stag = d->stagger;
    r.literal = r.anel || r.stag || dealias;
    r.pfilter = d->pressure_filter_set();
    r.forces = po ? po->forces : tail && tail->forces && d->force.any();
    r.scal_src = tail && tail->scal_sources && d->infrared_on();
    r.zone_flow = !po && d->buffer_any(0);
    r.zone_scal = tail && tail->scal_zones && ns > 0 && d->buffer_any(1);

    auto burgers_ok = [&](int dir, tlab_fdm_plan_t g) {
        return r.anel ? tlab_internal_burgers_fusable_anelastic(dir, g, nx, ny, nz) : tlab_internal_burgers_fusable(dir, g, nx, ny, nz);
    };
    r.batched = !dealias && d->fuse && burgers_ok(1, gx) && burgers_ok(2, gy) && burgers_ok(3, gz);
    r.acc_direct = d->fuse && !r.anel && !dealias;
    r.x_last = !finish_off && r.batched && !r.literal && tlab_internal_burgers_can_finish(1, gx, nx, ny, nz);
    const bool p1[3] = {tlab_internal_partial_p1_fusable(1, gx, nx, ny, nz), tlab_internal_partial_p1_fusable(2, gy, nx, ny, nz),
                        tlab_internal_partial_p1_fusable(3, gz, nx, ny, nz)};
    const bool can_v_final = tlab_internal_poisson_can_v_final(d->poisson);
    r.neu_fast = (r.any_q || scal_neu) && tail && d->fuse && !r.literal && nz > 1 && !r.pfilter && !r.any_surface && can_v_final &&
                 tlab_internal_neumann_final_ok(gy, nx, ny, nz) && p1[0] && p1[2];

    bool finish_scal = r.x_last && tail && ns > 0, planes = false;
    if (finish_scal && scal_neu && r.neu_fast && neu_planes) {
        planes = true;
        for (int is = 0; is < ns; ++is)
            if (r.ibc_s[is] != 0 && !neumann_weights(d, r.ibc_s[is])) planes = false;
    }
    for (int is = 0; is < ns && !planes; ++is) finish_scal = finish_scal && r.ibc_s[is] == 0;
    finish_scal = finish_scal && !r.any_surface;      // the wall planes of a scalar with a surface model are not zero
    // (zone_epi excludes a wall plane that BOTH blocks hold: the plane form restarts from the BC value, so it runs once per plane)
    const bool walls_shared = (d->buff[1][0].size == ny && d->buff[1][1].size > 0) || (d->buff[1][1].size == ny && d->buff[1][0].size > 0);
    r.zone_epi = r.zone_scal && finish_scal && !planes && !walls_shared;
    r.zone_tail = r.zone_scal && !r.zone_epi;
    r.finish_scal = finish_scal && !r.zone_tail;
    r.scal_neumann_planes = planes && !r.zone_tail;

    r.div_in_burgers = r.x_last && d->fuse && p1[1] && p1[2];
    r.div_all = r.div_in_burgers && nz > 1 && tlab_internal_burgers_can_div(2, gy, nx, ny, nz) && tlab_internal_burgers_can_div(3, gz, nx, ny, nz);
    r.fused_div = !r.literal && d->fuse && p1[0] && p1[1] && p1[2];
    for (int iq = 0; iq < 3; ++iq) r.flow_planes[iq] = iq != 1 && r.neu_fast && r.ibc_q[iq] != 0 && neu_planes && neumann_weights(d, r.ibc_q[iq]);
    r.v_final = tail && d->fuse && !r.literal && !r.pfilter && (r.walls_dirichlet || r.neu_fast) && can_v_final;
    const bool grad_fast = d->fuse && !r.literal && nz > 1 && p1[0] && p1[2];
    r.grad_final = tail && grad_fast && r.walls_dirichlet;
    r.grad_sub = grad_fast && !r.grad_final;
    for (int iq = 0; iq < 3; ++iq) r.gw_defer[iq] = r.anel && tail && d->fuse && r.ibc_q[iq] == 0;
    return r;
}

// What every stage needs of one substep, built once
struct Ctx {
    tlab_dns *d;
    const SubstepTail *tail;
    int nx, ny, nz;
    long long n;
    hipStream_t st;
    double dte, kco, idte;
    int scale;
    double *const *q, *const *s, *const *hq, *const *hs;
    double *const *vel;           // the advecting velocity of each direction: q, but for the diffusion part of a pressure decomposition (zeros)
    double *tmp1, *tmp2, *tmp3, *tmp4, *tmp5, *tmp7, *tmp8, *tmp9;      // txc(:,1:9) in the reference's roles
    tlab_fdm_plan_t gx, gy, gz;
    std::vector<tlab::ClipBounds> tail_clip;      // the bounds of the tail as the kernels take them
    Ctx(tlab_dns *d_, double dte_, double *const *q_, double *const *s_, double *const *hq_, double *const *hs_, double *const *txc, const SubstepTail *tail_,
        bool p_only = false, double *const *vel_ = nullptr)
        : d(d_), tail(tail_), nx(d_->nx), ny(d_->ny), nz(d_->nz), n((long long)d_->nx * d_->ny * d_->nz), st(tlab_current_stream()), dte(dte_),
          kco(tail_ ? tail_->kco : 1.0),
          idte(d_->remove_divergence && !p_only ? 1.0 / dte_ : 0.0),      // hq + 0 q is hq bit for bit: the same kernels serve the else-branch (:234-250)
          scale(tail_ ? tail_->scale : 0), q(q_), s(s_), hq(hq_), hs(hs_), vel(vel_ ? vel_ : q_), tmp1(txc[0]), tmp2(txc[1]), tmp3(txc[2]), tmp4(txc[3]), tmp5(txc[4]),
          tmp7(txc[6]), tmp8(txc[7]), tmp9(txc[8]), gx(d_->g[0]), gy(d_->g[1]), gz(d_->g[2]) {
        if (tail && tail->bounds)
            for (size_t is = 0; is < tail->bounds->on.size(); ++is) tail_clip.push_back({tail->bounds->lo[is], tail->bounds->hi[is]});
    }
    // the bounds of scalar is, or NULL when it is not limited
    const tlab::ClipBounds *clip_of(int is) const { return tail && tail->clips(is) ? &tail_clip[is] : nullptr; }
    size_t plane_bytes() const { return (size_t)nx * nz * sizeof(double); }
};

// keep the old tendency of the scalar at the boundary for the dynamic BCs (:77-87); zero otherwise.  Reads d->fresh: it runs before the flag is consumed.
void keep_surface_planes(const Ctx &c) {
    tlab_dns *d = c.d;
    for (int is = 0; is < d->nscal; ++is) {
        if (!d->surface(is)) continue;
        // at the start of a Runge-Kutta step the tendencies COUNT as zero (tlab_dns_begin_step instead of the fill of time.f90:212-216): whatever
        // hs still holds from the last step must not become BcsScal%ref
        if (d->fresh) {
            hk(hipMemsetAsync(d->sref_b[is], 0, c.plane_bytes(), c.st), "memset");
            hk(hipMemsetAsync(d->sref_t[is], 0, c.plane_bytes(), c.st), "memset");
            continue;
        }
        hk(launch_get_wall_planes(c.hs[is], d->sref_b[is], d->sref_t[is], c.nx, c.ny, c.nz, c.st), "wall planes");
        if (d->sfc_jmin[is] != 1) hk(hipMemsetAsync(d->sref_b[is], 0, c.plane_bytes(), c.st), "memset");
        if (d->sfc_jmax[is] != 1) hk(hipMemsetAsync(d->sref_t[is], 0, c.plane_bytes(), c.st), "memset");
    }
}

// ---- diffusion and advection (:98-136), scalars (:149-162).  Reference: every OPR_Burgers result goes to a tmp array and
// hq = hq + tmp_a + tmp_b + tmp_c afterwards; here each kernel adds its result to hq directly (same summation order)
// when the fused kernels apply, and falls back to tmp + k_add3 per equation otherwise. ----
struct Eq { double *dst; const double *fld; double nu; int order[3]; };   // order = directions in the reference's summation order
std::vector<Eq> equations(const Ctx &c, bool scalars = true) {
    const double nu = c.d->visc;
    std::vector<Eq> eqs = {{c.hq[0], c.q[0], nu, {1, 2, 3}},      // hq1 + tmp1(X) + tmp7(Y) + tmp8(Z)   (:110)
                           {c.hq[1], c.q[1], nu, {2, 1, 3}},      // hq2 + tmp2(Y) + tmp7(X) + tmp8(Z)   (:122)
                           {c.hq[2], c.q[2], nu, {3, 1, 2}}};     // hq3 + tmp3(Z) + tmp7(X) + tmp8(Y)   (:134)
    for (int is = 0; is < c.d->nscal && scalars; ++is) eqs.push_back({c.hs[is], c.s[is], c.d->visc / c.d->schmidt[is], {1, 2, 3}});   // :158, opr_burgers.f90:97
    return eqs;
}

// The slot in the middle of the Burgers sums, where every tendency holds a valid partial sum and none is finished:
// BOUNDARY_BUFFER_RELAX_FLOW (:170-172; the terms are summed in another order, rounding only), the zone term of scalars the x epilogue finishes, the
// body forces (q and s are those from before the update, and the forcing of the pressure and the wall planes of hq2 are formed later, so the force is
// projected) and the scalar source.  Five launches: after the second (every component has been overwritten once, the third finishes u and
// differentiates it).  Three launches: after the first (it may overwrite), before the last (it may differentiate).  Per-equation sums: after them,
// the reference's place.
void mid_sequence_terms(const Ctx &c, const Route &r) {
    if (r.zone_flow) buffer_relax(c.d, 0, c.q, c.hq, c.st);
    if (r.zone_epi) buffer_relax(c.d, 1, c.s, c.hs, c.st);
    if (r.forces) body_force(c.d, c.q, c.s, c.hq, c.st);
    if (r.scal_src) sources_scal(c.d, c.s, c.hs, c.tmp8, c.tmp9, c.st);
}

// One launch of the equations eq[0 .. nf) (at most four) along dir.  finishing: the launch adds the last term of its scalars (equations 3..), and
// finishes them where the route says so.  overwrite / fresh_mask: all / some of its fields start their tendency here.  divp: where the launch
// adds the forcing term of its first field, or NULL.
void burgers_batch(const Ctx &c, const Route &r, const std::vector<Eq> &eqs, int dir, const int *eq, int nf, bool finishing, bool overwrite,
                   unsigned fresh_mask, double *divp) {
    const double *sp[4]; double *rp[4]; double nup[4];
    int fin[4] = {0, 0, 0, 0}, clip[4] = {0, 0, 0, 0};
    double clo[4] = {0, 0, 0, 0}, chi[4] = {0, 0, 0, 0};
    for (int f = 0; f < nf; ++f) {
        const int e = eq[f], is = eq[f] - 3;
        sp[f] = eqs[e].fld; rp[f] = eqs[e].dst; nup[f] = eqs[e].nu;
        fin[f] = (r.finish_scal && finishing && is >= 0) ? 1 : 0;
        // scalar bounds in the epilogue that finishes the scalar: on every line, or -- Neumann walls on the wall-plane route -- on the interior lines,
        // k_wall_fix clipping the wall planes once they are set
        if (const tlab::ClipBounds *cl = fin[f] ? c.clip_of(is) : nullptr) {
            clip[f] = (r.scal_neumann_planes && r.ibc_s[is] != 0) ? 2 : 1;
            clo[f] = cl->lo; chi[f] = cl->hi;
        }
    }
    const bool any_fin = fin[0] || fin[1] || fin[2] || fin[3];
    const bool any_clip = clip[0] || clip[1] || clip[2] || clip[3];
    if (!tlab_internal_burgers_acc_n(dir, c.d->g[dir - 1], c.nx, c.ny, c.nz, 0, nf, nup, sp, c.vel[dir - 1], rp, overwrite, any_fin ? fin : nullptr, c.dte,
                                     c.kco, c.scale ? 1 : 0, divp, c.idte, fresh_mask, r.anel ? c.d->rib : nullptr, any_clip ? clip : nullptr, clo, chi))
        throw Fail(TLAB_EINVAL, "internal: inconsistent fused Burgers path");
}

// div_all: z (all but w), y (all but v), x (all), y (v), z (w).  fresh: TIME_RUNGEKUTTA zeroes hq, hs at the start of a step (time.f90:212-216) --
// the first launch of each field overwrites instead
void burgers_five_launches(const Ctx &c, const Route &r, const std::vector<Eq> &eqs, bool fresh) {
    struct Launch { int dir; std::vector<int> eq; bool last_x; int divf; };      // divf: equation whose forcing term rides on the launch (-1: none)
    std::vector<int> all_but_w, all_but_v, all;
    for (int e = 0; e < (int)eqs.size(); ++e) { all.push_back(e); if (e != 2) all_but_w.push_back(e); if (e != 1) all_but_v.push_back(e); }
    const Launch plan[5] = {{3, all_but_w, false, -1}, {2, all_but_v, false, -1}, {1, all, true, 0}, {2, {1}, false, 1}, {3, {2}, false, 2}};
    bool touched[16] = {false};
    for (const Launch &L : plan) {
        for (size_t e0 = 0; e0 < L.eq.size(); e0 += 4) {
            const int nf = (int)std::min<size_t>(4, L.eq.size() - e0);
            unsigned fresh_mask = 0;
            bool all_fresh = fresh, any_fresh = false;
            for (int f = 0; f < nf; ++f) {
                const int e = L.eq[e0 + f];
                if (fresh && !touched[e]) { fresh_mask |= 1u << f; any_fresh = true; } else all_fresh = false;
                touched[e] = true;
            }
            const bool over = all_fresh && any_fresh;                   // every field of the launch starts its tendency here
            const bool div = L.divf >= 0 && (L.dir != 1 || e0 == 0);    // x: batch 0 holds u; y, z: the one-field launches
            burgers_batch(c, r, eqs, L.dir, &L.eq[e0], nf, L.last_x, over, over ? 0u : fresh_mask, div ? c.tmp1 : nullptr);
        }
        if (&L == &plan[1]) mid_sequence_terms(c, r);
    }
}

// batched without div_all: one launch per direction and batch of four, x last where it can finish the scalars or write the x term of the forcing
void burgers_three_launches(const Ctx &c, const Route &r, const std::vector<Eq> &eqs, bool fresh) {
    std::vector<int> all(eqs.size());
    for (size_t e = 0; e < eqs.size(); ++e) all[e] = (int)e;
    for (int k = 0; k < 3; ++k) {
        const int dir = r.x_last ? 3 - k : 1 + k;
        for (size_t e0 = 0; e0 < eqs.size(); e0 += 4)      // (batch 0 holds u)
            burgers_batch(c, r, eqs, dir, &all[e0], (int)std::min<size_t>(4, eqs.size() - e0), k == 2, fresh && k == 0, 0u,
                          (r.div_in_burgers && dir == 1 && e0 == 0) ? c.tmp1 : nullptr);
        if (k == 0) mid_sequence_terms(c, r);
    }
}

// the reference's sums, equation by equation: each term added by its launch where the fast kernels apply, otherwise through tmp1 / tmp7 / tmp8 + k_add3
void burgers_per_equation(const Ctx &c, const Route &r, const std::vector<Eq> &eqs, bool fresh) {
    tlab_dns *d = c.d;
    if (fresh)
        for (const Eq &e : eqs) hk(hipMemsetAsync(e.dst, 0, (size_t)c.n * sizeof(double), c.st), "memset");
    double *tmps[3] = {c.tmp1, c.tmp7, c.tmp8};
    for (const Eq &e : eqs) {
        double *pend[3];
        int npend = 0;
        for (int k = 0; k < 3; ++k) {
            const int dir = e.order[k];
            const double *vel = c.vel[dir - 1];
            if (r.acc_direct && tlab_internal_burgers_acc(dir, d->g[dir - 1], c.nx, c.ny, c.nz, 0, e.nu, e.fld, vel, e.dst)) continue;
            ok(tlab_opr_burgers(dir, d->g[dir - 1], e.fld == vel ? TLAB_OPR_B_SELF : TLAB_OPR_B_U_IN, c.nx, c.ny, c.nz, 0, e.nu, e.fld, vel, tmps[k], c.tmp9, 0),
               "OPR_Burgers");
            pend[npend++] = tmps[k];
        }
        if (npend == 3) hk(launch_add3(e.dst, pend[0], pend[1], pend[2], c.n, c.st), "add3");
        else if (npend > 0) {   // mixed: add the temporaries one at a time (k_add3 with zero-sized partners is not worth a kernel)
            hk(hipMemsetAsync(c.tmp9, 0, (size_t)c.n * sizeof(double), c.st), "memset");
            hk(launch_add3(e.dst, pend[0], npend > 1 ? pend[1] : c.tmp9, c.tmp9, c.n, c.st), "add3");
        }
    }
    mid_sequence_terms(c, r);      // (the tendencies were zeroed or accumulated above; the forcing follows)
}

void burgers_sums(const Ctx &c, const Route &r, const std::vector<Eq> &eqs, bool fresh) {
    if (r.div_all) burgers_five_launches(c, r, eqs, fresh);
    else if (r.batched) burgers_three_launches(c, r, eqs, fresh);
    else burgers_per_equation(c, r, eqs, fresh);
}

// the tail of the scalars under a buffer zone, once the wall planes of hs hold their BC values: BOUNDARY_BUFFER_RELAX_SCAL, s += dte hs, bounds, hs *= kco
void zone_scal_tail(const Ctx &c) {
    buffer_relax(c.d, 1, c.s, c.hs, c.st);
    for (int is = 0; is < c.d->nscal; ++is) hk(launch_rk_update(c.s[is], c.hs[is], c.dte, c.kco, c.scale, c.n, c.st, c.clip_of(is)), "rk update");
}

// zone_epi: the wall planes inside the zones, after the epilogue that finished the rest (nothing later reads s or hs)
void zone_wall_planes(const Ctx &c) {
    for (int end = 0; end < 2; ++end) {
        const tlab_dns::BufferBlock &b = c.d->buff[1][end];
        if (b.size == 0) continue;
        const long long zone = (long long)c.nx * b.size * c.nz;
        for (int f0 = 0; f0 < b.nf; f0 += 4) {
            const tlab::ClipBounds *cl[4] = {nullptr, nullptr, nullptr, nullptr};
            for (int f = f0; f < std::min(b.nf, f0 + 4); ++f) cl[f - f0] = c.clip_of(f);
            // the wall plane the block starts from, and the opposite one where the block spans the whole height (tau need not vanish there: sigma = 0)
            for (int wall = 0; wall < 2; ++wall) {
                const int j = wall == 0 ? 0 : c.ny - 1;
                if (j < b.offset || j >= b.offset + b.size) continue;
                hk(launch_buffer_relax_plane(std::min(4, b.nf - f0), c.hs + f0, c.s + f0, b.ref + f0 * zone, b.tau + (long long)f0 * b.size, nullptr, cl, c.dte,
                                             c.kco, c.scale, c.nx, c.ny, c.nz, b.offset, b.size, j - b.offset, c.st), "buffer zone (wall plane)");
            }
        }
    }
}

// the forcing as the reference forms it: tmp2 | tmp3 | tmp4 = hq + q / dte, three derivatives, their sum in tmp1
void pressure_forcing_literal(const Ctx &c, const Route &r) {
    tlab_dns *d = c.d;
    const int nx = c.nx, ny = c.ny, nz = c.nz;
    double *tmp1 = c.tmp1, *tmp2 = c.tmp2, *tmp3 = c.tmp3, *tmp4 = c.tmp4, *tmp5 = c.tmp5;
    if (r.anel && d->fuse) {      // ... with Thermo_Anelastic_WEIGHT_INPLACE(.., rbackground, tmp2 | tmp3 | tmp4) (:211-214) in the same pass
        hk(launch_axpy3w(tmp2, tmp3, tmp4, c.hq[1], c.hq[0], c.hq[2], c.q[1], c.q[0], c.q[2], c.idte, d->rb, nx, ny, c.n, c.st), "axpy3w");
    } else {
        hk(launch_axpy3(tmp2, tmp3, tmp4, c.hq[1], c.hq[0], c.hq[2], c.q[1], c.q[0], c.q[2], c.idte, c.n, c.st), "axpy3");
        if (r.anel) {      // Thermo_Anelastic_WEIGHT_INPLACE(.., rbackground, tmp2 | tmp3 | tmp4)  (:211-214)
            hk(launch_weight_y(tmp2, tmp2, d->rb, nx, ny, c.n, 0, c.st), "weight");
            hk(launch_weight_y(tmp3, tmp3, d->rb, nx, ny, c.n, 0, c.st), "weight");
            hk(launch_weight_y(tmp4, tmp4, d->rb, nx, ny, c.n, 0, c.st), "weight");
        }
    }
    if (r.stag) {      // the three terms on the horizontal pressure nodes (:216-226)
        ok(tlab_opr_partial(1, c.gx, TLAB_OPR_P0_INT_VP, nx, ny, nz, B0, tmp2, tmp5, nullptr), "OPR_Partial_X(P0_INT_VP)");      // Oy derivative
        ok(tlab_opr_partial(2, c.gy, TLAB_OPR_P1, nx, ny, nz, B0, tmp5, tmp2, nullptr), "OPR_Partial_Y");
        ok(tlab_opr_partial(3, c.gz, TLAB_OPR_P0_INT_VP, nx, ny, nz, B0, tmp2, tmp1, nullptr), "OPR_Partial_Z(P0_INT_VP)");
        ok(tlab_opr_partial(1, c.gx, TLAB_OPR_P1_INT_VP, nx, ny, nz, B0, tmp3, tmp5, nullptr), "OPR_Partial_X(P1_INT_VP)");      // Ox derivative
        ok(tlab_opr_partial(3, c.gz, TLAB_OPR_P0_INT_VP, nx, ny, nz, B0, tmp5, tmp2, nullptr), "OPR_Partial_Z(P0_INT_VP)");
        ok(tlab_opr_partial(1, c.gx, TLAB_OPR_P0_INT_VP, nx, ny, nz, B0, tmp4, tmp5, nullptr), "OPR_Partial_X(P0_INT_VP)");      // Oz derivative
        ok(tlab_opr_partial(3, c.gz, TLAB_OPR_P1_INT_VP, nx, ny, nz, B0, tmp5, tmp3, nullptr), "OPR_Partial_Z(P1_INT_VP)");
    } else {
        ok(tlab_opr_partial(2, c.gy, TLAB_OPR_P1, nx, ny, nz, B0, tmp2, tmp1, nullptr), "OPR_Partial_Y");
        ok(tlab_opr_partial(1, c.gx, TLAB_OPR_P1, nx, ny, nz, B0, tmp3, tmp2, nullptr), "OPR_Partial_X");
        ok(tlab_opr_partial(3, c.gz, TLAB_OPR_P1, nx, ny, nz, B0, tmp4, tmp3, nullptr), "OPR_Partial_Z");
    }
    hk(launch_sum3(tmp1, tmp2, tmp3, c.n, c.st), "sum3");
}

// ---- pressure (:177-260, remove_divergence branch): forcing = div(hq + q/dte) in tmp1 ----
void pressure_forcing(const Ctx &c, const Route &r) {
    const int nx = c.nx, ny = c.ny, nz = c.nz;
    auto term = [&](int dir, tlab_fdm_plan_t g, int iq, bool acc) {
        return tlab_internal_partial_p1_fused(dir, g, nx, ny, nz, B0, c.hq[iq], c.q[iq], c.idte, c.tmp1, acc);
    };
    if (r.div_all) return;      // tmp1 holds the three terms
    if (r.div_in_burgers) {     // tmp1 holds the x term already
        if (!term(2, c.gy, 1, true) || !term(3, c.gz, 2, true)) throw Fail(TLAB_EINVAL, "internal: inconsistent fused divergence path");
        return;
    }
    if (r.fused_div && term(2, c.gy, 1, false)) {      // (the y launch declines: nothing is written, the literal sequence serves)
        if (!term(1, c.gx, 0, true) || !term(3, c.gz, 2, true)) throw Fail(TLAB_EINVAL, "internal: inconsistent fused divergence path");
        return;
    }
    pressure_forcing_literal(c, r);
}

// the wall planes of hq2, the solve, the pressure filter: pressure in tmp1, its Oy derivative in tmp3 unless the solver finishes v (v_final)
void pressure_solve(const Ctx &c, const Route &r) {
    tlab_dns *d = c.d;
    const int nx = c.nx, ny = c.ny, nz = c.nz;
    // Neumann BCs in d/dy(p) s.t. v = 0 (:263-281); staggered: the planes of hq2 interpolated onto the pressure nodes (:266-269)
    if (r.stag) {
        ok(tlab_opr_partial(1, c.gx, TLAB_OPR_P0_INT_VP, nx, ny, nz, B0, c.hq[1], c.tmp5, nullptr), "OPR_Partial_X(P0_INT_VP)");
        ok(tlab_opr_partial(3, c.gz, TLAB_OPR_P0_INT_VP, nx, ny, nz, B0, c.tmp5, c.tmp4, nullptr), "OPR_Partial_Z(P0_INT_VP)");
    }
    hk(launch_get_wall_planes(r.stag ? c.tmp4 : c.hq[1], d->bcs_hb, d->bcs_ht, nx, ny, nz, c.st), "wall planes");
    if (r.anel) {          // BcsFlowJmin%ref(:,:,2) = p_bcs(:,1,:) * rbackground(1), Jmax likewise (:275-277)
        hk(launch_scale(d->bcs_hb, d->rb_wall[0], (long long)nx * nz, c.st), "scale");
        hk(launch_scale(d->bcs_ht, d->rb_wall[1], (long long)nx * nz, c.st), "scale");
    }
    if (r.v_final) tlab_internal_poisson_arm_v_final(d->poisson, c.q[1], c.hq[1], c.dte, c.kco, c.scale);
    ok(tlab_opr_poisson(d->poisson, nx, ny, nz, TLAB_BCS_NN, c.tmp1, c.tmp2, c.tmp4, d->bcs_hb, d->bcs_ht, r.p_only ? nullptr : c.tmp3), "OPR_Poisson");
    if (r.pfilter) {      // filter pressure p and its vertical gradient dpdy (:286-290)
        ok(tlab_opr_filter(nx, ny, nz, d->pfilter[0], d->pfilter[1], d->pfilter[2], d->pfilter_rep, c.tmp1, c.tmp4), "OPR_FILTER(p)");
        if (!r.p_only) ok(tlab_opr_filter(nx, ny, nz, d->pfilter[0], d->pfilter[1], d->pfilter[2], d->pfilter_rep, c.tmp3, c.tmp4), "OPR_FILTER(dpdy)");
    }
}

// the taps of the towers and the phase averages (:292-305), armed by tlab_dns_arm_pressure_sampling: the pressure in tmp1, on the staggered grid its
// image on the velocity nodes in tmp4 through tmp5 (both free between the solve and the gradient, :294-297).  Where the grid is not staggered the
// reference hands over tmp4, the solver's work array; the pressure is sampled here.
void pressure_taps(const Ctx &c, const Route &r, const tlab_dns::PressureSampling &ps) {
    const double *p = c.tmp1;
    if (r.stag) {
        ok(tlab_opr_partial(3, c.gz, TLAB_OPR_P0_INT_PV, c.nx, c.ny, c.nz, B0, c.tmp1, c.tmp5, nullptr), "OPR_Partial_Z(P0_INT_PV)");
        ok(tlab_opr_partial(1, c.gx, TLAB_OPR_P0_INT_PV, c.nx, c.ny, c.nz, B0, c.tmp5, c.tmp4, nullptr), "OPR_Partial_X(P0_INT_PV)");
        p = c.tmp4;
    }
    pressure_sampling(c.d, ps, p);
}

// six planes of scratch for the weighted sums next to the walls, allocated on first use
double *wall_planes(const Ctx &c) {
    if (!c.d->wall_planes) hk(hipMalloc((void **)&c.d->wall_planes, 6 * c.plane_bytes()), "hipMalloc");
    return c.d->wall_planes;
}

// neu_fast: everything after the solve with a Neumann wall somewhere -- u along x, w along z, then the scalars (v is finished by the solver)
void neumann_fast_tail(const Ctx &c, const Route &r) {
    tlab_dns *d = c.d;
    const int nx = c.nx, ny = c.ny, nz = c.nz, scale = c.scale;
    const double dte = c.dte, kco = c.kco;
    const size_t np = (size_t)nx * nz;
    for (int iq = 0; iq < 3; iq += 2) {
        const int dir = iq == 0 ? 1 : 3;
        tlab_fdm_plan_t gd = iq == 0 ? c.gx : c.gz;
        const int ibc = r.ibc_q[iq];
        bool done;
        if (ibc == 0) done = tlab_internal_gradient_final(dir, gd, nx, ny, nz, c.tmp1, c.q[iq], c.hq[iq], dte, kco, scale);
        else if (r.flow_planes[iq]) {
            // wall tendencies from weighted sums over the rows next to the walls (of hq and of p; the derivative of the p planes commutes
            // with the sum), then the gradient kernel finishes the field as it does with Dirichlet walls -- one pass over hq instead of two
            const tlab_dns::NeuW &W = d->neuw[ibc];
            double *Hb = wall_planes(c), *Ht = Hb + np, *Pb = Ht + np, *Pt = Pb + np, *Db = Pt + np, *Dt = Db + np;
            hk(launch_wall_weighted(c.hq[iq], c.tmp1, W.w, W.w + W.K, W.K, Hb, Ht, Pb, Pt, nx, ny, nz, c.st), "wall planes");
            ok(tlab_opr_partial(dir, gd, TLAB_OPR_P1, nx, 1, nz, 0, Pb, Db, nullptr), "OPR_Partial (wall plane)");
            ok(tlab_opr_partial(dir, gd, TLAB_OPR_P1, nx, 1, nz, 0, Pt, Dt, nullptr), "OPR_Partial (wall plane)");
            hk(launch_sub2(Hb, Hb, Db, (long long)np, c.st), "wall planes");
            hk(launch_sub2(Ht, Ht, Dt, (long long)np, c.st), "wall planes");
            done = tlab_internal_gradient_final(dir, gd, nx, ny, nz, c.tmp1, c.q[iq], c.hq[iq], dte, kco, scale, (ibc & 1) ? Hb : nullptr,
                                                (ibc & 2) ? Ht : nullptr);
        } else done = tlab_internal_partial_p1_sub(dir, gd, nx, ny, nz, c.tmp1, c.hq[iq]) &&
                      tlab_internal_neumann_final(c.gy, nx, ny, nz, ibc, c.hq[iq], c.q[iq], dte, kco, scale);
        if (!done) throw Fail(TLAB_EINVAL, "internal: inconsistent fused Neumann tail");
    }
    if (r.zone_tail) {      // (tmp1 and the two planes are free: u, v, w are finished)
        for (int is = 0; is < d->nscal; ++is) {
            const int ibc = r.ibc_s[is];
            if (ibc != 0) ok(tlab_boundary_bcs_neumann_y(c.gy, ibc, nx, ny, nz, c.hs[is], d->bcs_hb, d->bcs_ht, c.tmp1), "BOUNDARY_BCS_NEUMANN_Y");
            hk(launch_set_wall_planes(c.hs[is], (ibc & 1) ? d->bcs_hb : nullptr, (ibc & 2) ? d->bcs_ht : nullptr, nx, ny, nz, c.st), "wall planes");
        }
        zone_scal_tail(c);
    }
    for (int is = 0; is < d->nscal && !r.finish_scal && !r.zone_tail; ++is) {
        const int ibc = r.ibc_s[is];
        if (ibc == 0) hk(launch_final_update(c.s[is], c.hs[is], nullptr, nullptr, nullptr, dte, kco, scale, nx, ny, nz, c.st, nullptr, c.clip_of(is)),
                         "final update");
        else if (!tlab_internal_neumann_final(c.gy, nx, ny, nz, ibc, c.hs[is], c.s[is], dte, kco, scale))
            throw Fail(TLAB_EINVAL, "internal: inconsistent fused Neumann tail");
        else if (const tlab::ClipBounds *cl = c.clip_of(is))      // (the y-line tail kernel has no bounds epilogue: a pass of its own)
            hk(launch_clip(c.s[is], cl->lo, cl->hi, c.n, c.st), "clip");
    }
    for (int is = 0; is < d->nscal && r.finish_scal && r.scal_neumann_planes; ++is) {      // finished by the x Burgers launch but for their wall planes
        const int ibc = r.ibc_s[is];
        if (ibc == 0) continue;
        const tlab_dns::NeuW &W = d->neuw[ibc];
        double *Sb = wall_planes(c), *St = Sb + np;
        hk(launch_wall_weighted(c.hs[is], nullptr, W.w, W.w + W.K, W.K, Sb, St, nullptr, nullptr, nx, ny, nz, c.st), "wall planes");
        hk(launch_wall_fix(c.s[is], c.hs[is], (ibc & 1) ? Sb : nullptr, (ibc & 2) ? St : nullptr, dte, kco, scale, nx, ny, nz, c.st, c.clip_of(is)),
           "wall planes");
    }
}

// ---- pressure gradient (:319-320): u and w finished by the gradient kernels, or the gradient subtracted by its own launches, or dp/dx, dp/dy,
// dp/dz stored in tmp2, tmp3, tmp4 for the update (the staggered branch: back onto the horizontal velocity nodes) ----
void pressure_gradient(const Ctx &c, const Route &r) {
    const int nx = c.nx, ny = c.ny, nz = c.nz;
    double *tmp1 = c.tmp1, *tmp2 = c.tmp2, *tmp3 = c.tmp3, *tmp4 = c.tmp4, *tmp5 = c.tmp5;
    if (r.grad_final) {
        if (!tlab_internal_gradient_final(1, c.gx, nx, ny, nz, tmp1, c.q[0], c.hq[0], c.dte, c.kco, c.scale) ||
            !tlab_internal_gradient_final(3, c.gz, nx, ny, nz, tmp1, c.q[2], c.hq[2], c.dte, c.kco, c.scale))
            throw Fail(TLAB_EINVAL, "internal: inconsistent fused gradient path");
    } else if (r.grad_sub) {
        if (!tlab_internal_partial_p1_sub(1, c.gx, nx, ny, nz, tmp1, c.hq[0]) || !tlab_internal_partial_p1_sub(3, c.gz, nx, ny, nz, tmp1, c.hq[2]))
            throw Fail(TLAB_EINVAL, "internal: inconsistent fused gradient path");
        if (!r.v_final) hk(launch_axpy1(c.hq[1], c.hq[1], tmp3, -1.0, c.n, c.st), "axpy1");      // hq2 - dp/dy
    } else if (r.stag) {          // back onto the horizontal velocity nodes (:307-317)
        ok(tlab_opr_partial(3, c.gz, TLAB_OPR_P0_INT_PV, nx, ny, nz, B0, tmp3, tmp5, nullptr), "OPR_Partial_Z(P0_INT_PV)");       // dp/dy
        ok(tlab_opr_partial(1, c.gx, TLAB_OPR_P0_INT_PV, nx, ny, nz, B0, tmp5, tmp3, nullptr), "OPR_Partial_X(P0_INT_PV)");
        ok(tlab_opr_partial(3, c.gz, TLAB_OPR_P1_INT_PV, nx, ny, nz, B0, tmp1, tmp5, nullptr), "OPR_Partial_Z(P1_INT_PV)");       // dp/dz
        ok(tlab_opr_partial(1, c.gx, TLAB_OPR_P0_INT_PV, nx, ny, nz, B0, tmp5, tmp4, nullptr), "OPR_Partial_X(P0_INT_PV)");
        ok(tlab_opr_partial(3, c.gz, TLAB_OPR_P0_INT_PV, nx, ny, nz, B0, tmp1, tmp5, nullptr), "OPR_Partial_Z(P0_INT_PV)");       // dp/dx
        ok(tlab_opr_partial(1, c.gx, TLAB_OPR_P1_INT_PV, nx, ny, nz, B0, tmp5, tmp2, nullptr), "OPR_Partial_X(P1_INT_PV)");
    } else {
        ok(tlab_opr_partial(1, c.gx, TLAB_OPR_P1, nx, ny, nz, B0, tmp1, tmp2, nullptr), "OPR_Partial_X(p)");
        ok(tlab_opr_partial(3, c.gz, TLAB_OPR_P1, nx, ny, nz, B0, tmp1, tmp4, nullptr), "OPR_Partial_Z(p)");
    }
}

// ---- boundary conditions (:360-398): Dirichlet -> the tendency vanishes on the wall plane; Neumann -> the wall tendency
// keeps d/dy = 0 there (BOUNDARY_BCS_NEUMANN_Y on the finished tendency; tmp1 is its work array as in the reference) ----
// planes of a field: Neumann values where selected, zeros (null) elsewhere
void neumann_planes(const Ctx &c, int ibc, const double *h, const double *&pb, const double *&pt) {
    pb = pt = nullptr;
    if (ibc == 0) return;
    ok(tlab_boundary_bcs_neumann_y(c.gy, ibc, c.nx, c.ny, c.nz, h, c.d->bcs_hb, c.d->bcs_ht, c.tmp1), "BOUNDARY_BCS_NEUMANN_Y");
    if (ibc & 1) pb = c.d->bcs_hb;
    if (ibc & 2) pt = c.d->bcs_ht;
}
// planes of a scalar: Neumann values where selected, then the dynamic surface model (BOUNDARY_BCS_SURFACE_Y, :393-396), zeros (null) elsewhere
void scalar_planes(const Ctx &c, const Route &r, int is, const double *&qb, const double *&qt) {
    tlab_dns *d = c.d;
    neumann_planes(c, r.ibc_s[is], c.hs[is], qb, qt);
    if (!d->surface(is)) return;
    if (qb) hk(hipMemcpyAsync(d->sref_b[is], qb, c.plane_bytes(), hipMemcpyDeviceToDevice, c.st), "memcpy");      // the Neumann value replaces the kept tendency
    if (qt) hk(hipMemcpyAsync(d->sref_t[is], qt, c.plane_bytes(), hipMemcpyDeviceToDevice, c.st), "memcpy");
    const double diff = d->visc / d->schmidt[is];
    ok(tlab_opr_partial(2, c.gy, TLAB_OPR_P1, c.nx, c.ny, c.nz, B0, c.s[is], c.tmp1, nullptr), "OPR_Partial_Y (surface flux)");      // boundary_bcs.f90:508
    // AVG1V2D(imax, jmax, kmax, 1, 1, tmp1) at BOTH ends (:520, :535): the plane j = 1
    if (d->sfc_jmin[is] == 1) hk(launch_surface_flux(d->sref_b[is], c.tmp1, 0, 0, 1.0, diff, d->cpl_jmin[is], d->sfc_avg, c.nx, c.ny, c.nz, c.st), "surface flux");
    if (d->sfc_jmax[is] == 1) hk(launch_surface_flux(d->sref_t[is], c.tmp1, c.ny - 1, 0, -1.0, diff, d->cpl_jmax[is], d->sfc_avg, c.nx, c.ny, c.nz, c.st), "surface flux");
    qb = d->sref_b[is]; qt = d->sref_t[is];
}

// the substep: hq -= grad p (:348-352), wall planes (:373-375), q += dte hq (time.f90:645-664), hq *= kco (:272-297) in one pass per field
void boundary_conditions_and_update(const Ctx &c, const Route &r) {
    const int nx = c.nx, ny = c.ny, nz = c.nz;
    double *gt[3] = {c.tmp2, c.tmp3, c.tmp4};
    bool subtracted = r.anel || r.grad_sub;      // subtracted before (anelastic: with the density weight)
    if (r.any_q && !subtracted) {   // the Neumann planes need the finished tendency first
        hk(launch_sub3(c.hq[0], c.hq[1], c.hq[2], c.tmp2, c.tmp3, c.tmp4, c.n, c.st), "sub3");
        subtracted = true;
    }
    const double *pb, *pt;
    for (int iq = 0; iq < 3; ++iq) {
        if (r.grad_final && iq != 1) continue;          // u and w are finished already
        if (r.v_final && iq == 1) continue;             // v too (inside OPR_Poisson)
        neumann_planes(c, r.ibc_q[iq], c.hq[iq], pb, pt);
        if (r.gw_defer[iq]) hk(launch_final_update(c.q[iq], c.hq[iq], gt[iq], pb, pt, c.dte, c.kco, c.scale, nx, ny, nz, c.st, c.d->rib), "final update");
        else hk(launch_final_update(c.q[iq], c.hq[iq], subtracted ? nullptr : gt[iq], pb, pt, c.dte, c.kco, c.scale, nx, ny, nz, c.st), "final update");
    }
    for (int is = 0; is < c.d->nscal && !r.finish_scal; ++is) {      // (finish_scal: done in the epilogue of the x Burgers launch)
        scalar_planes(c, r, is, pb, pt);
        if (r.zone_tail) hk(launch_set_wall_planes(c.hs[is], pb, pt, nx, ny, nz, c.st), "wall planes");
        else hk(launch_final_update(c.s[is], c.hs[is], nullptr, pb, pt, c.dte, c.kco, c.scale, nx, ny, nz, c.st, nullptr, c.clip_of(is)), "final update");
    }
    if (r.zone_tail) zone_scal_tail(c);
}

// the RHS on its own: the gradient subtracted, the wall planes set
void boundary_conditions_rhs_only(const Ctx &c, const Route &r) {
    const double *pb, *pt;
    if (!r.anel && !r.grad_sub) hk(launch_sub3(c.hq[0], c.hq[1], c.hq[2], c.tmp2, c.tmp3, c.tmp4, c.n, c.st), "sub3");
    for (int iq = 0; iq < 3; ++iq) {
        neumann_planes(c, r.ibc_q[iq], c.hq[iq], pb, pt);
        hk(launch_set_wall_planes(c.hq[iq], pb, pt, c.nx, c.ny, c.nz, c.st), "wall planes");
    }
    for (int is = 0; is < c.d->nscal; ++is) {
        scalar_planes(c, r, is, pb, pt);
        hk(launch_set_wall_planes(c.hs[is], pb, pt, c.nx, c.ny, c.nz, c.st), "wall planes");
    }
}
}  // namespace

void tlab::rhs_substep(tlab_dns *d, double dte, double *const *q, double *const *s, double *const *hq, double *const *hs, double *const *txc,
                       const SubstepTail *tail) {
    const tlab_dns::PressureSampling taps = d->psample;      // one-shot: cleared when taken, so an error below clears it too
    d->psample = tlab_dns::PressureSampling();
    const Ctx c(d, dte, q, s, hq, hs, txc, tail);
    follow_anelastic(d);
    keep_surface_planes(c);
    const bool fresh = d->fresh;       // one-shot (tlab_dns_begin_step): consumed here, after the stage that reads it and before the route, whose one
    d->fresh = false;                  // side effect may throw
    const Route r = decide_route(d, tail);
    const std::vector<Eq> eqs = equations(c);

    burgers_sums(c, r, eqs, fresh);
    if (r.zone_epi) zone_wall_planes(c);
    pressure_forcing(c, r);
    pressure_solve(c, r);
    if (taps.armed) pressure_taps(c, r, taps);
    if (r.scal_neumann_planes && !r.neu_fast) throw Fail(TLAB_EINVAL, "internal: Neumann scalars were finished without their wall planes");
    if (r.neu_fast) {
        neumann_fast_tail(c, r);
        return;
    }
    pressure_gradient(c, r);
    if (r.anel) {      // Thermo_Anelastic_WEIGHT_SUBTRACT (:326-329), unless the update of the component takes the weighted gradient as its operand
        double *gt[3] = {c.tmp2, c.tmp3, c.tmp4};
        for (int iq = 0; iq < 3; ++iq)
            if (!r.gw_defer[iq]) hk(launch_weight_y(hq[iq], gt[iq], d->rib, c.nx, c.ny, c.n, 1, c.st), "weight");
    }
    if (tail) boundary_conditions_and_update(c, r);
    else boundary_conditions_rhs_only(c, r);
}

// ---- FI_PRESSURE_BOUSSINESQ (physics/fi_pressure_boussinesq.f90:8-280): the stages above up to the solve, on three sums that are the caller's
// work arrays instead of the tendencies.  tmp[0..2] take the place of hq (they count as fresh: the first launch of each overwrites), p that of the
// forcing array tmp1, the caller's tmp1 | tmp2 that of the solver's work arrays tmp2 | tmp4; idte = 0 (no q / dte in the forcing), no scalar
// equation, no buffer zone, no tail.  What a route needs beyond that -- the sums of the literal forcing, the interpolation array of the staggered
// grid, the temporaries of the per-equation Burgers sums -- is the driver's own scratch, allocated on first use and kept.  Nothing of the driver's
// state is read that a substep consumes (d->fresh) and nothing is written but that scratch and the two wall planes every solve overwrites.
namespace {
enum { PW_TMP3, PW_TMP5, PW_TMP7, PW_TMP8, PW_TMP9 };      // the slots of tlab_dns::pwork, by the role of rhs_global_incompressible_1.f90
double *pressure_work(tlab_dns *d, int slot) {
    if (!d->pwork[slot]) hk(hipMalloc((void **)&d->pwork[slot], (size_t)(d->nx + 2) * d->ny * d->nz * sizeof(double)), "hipMalloc(pressure scratch)");
    return d->pwork[slot];
}
}  // namespace

void tlab::pressure_boussinesq(tlab_dns *d, int dcmp, double *const *q, double *const *s, double *p, double *tmp1, double *tmp2, double *const *tmp) {
    if (d->psample.armed) {      // the route that stops at the pressure has no tap: the arm is for a substep
        d->psample = tlab_dns::PressureSampling();
        throw Fail(TLAB_EUNSUPPORTED, "tlab_dns_pressure: a pressure sampling is armed (tlab_dns_arm_pressure_sampling serves the substep and the RHS)");
    }
    follow_anelastic(d);
    const bool total = dcmp == TLAB_DCMP_TOTAL, burgers = total || dcmp == TLAB_DCMP_ADVDIFF || dcmp == TLAB_DCMP_ADVECTION || dcmp == TLAB_DCMP_DIFFUSION;
    if (dcmp == TLAB_DCMP_BUOYANCY && d->bback && (d->force.g[0] != 0.0 || d->force.g[2] != 0.0))
        throw Fail(TLAB_EUNSUPPORTED, "tlab_dns_pressure: DCMP_BUOYANCY with a horizontal gravity component and a non-zero bbackground (the reference "
                                      "subtracts bbackground for the y component only there, fi_pressure_boussinesq.f90:171-177; the device holds one profile)");
    const PressureOnly po{total && d->force.any()};
    Route r = decide_route(d, nullptr, &po);
    // Only the plain Burgers sums of ONE pass can carry the forcing terms on their launches (the epilogue differentiates the tendency of the field
    // that is the advecting velocity of the launch): the difference of two passes (advection), the sums under a zero velocity (diffusion) and the
    // body forces on their own are differentiated afterwards, by the fused forcing launches where they apply
    if (dcmp != TLAB_DCMP_TOTAL && dcmp != TLAB_DCMP_ADVDIFF) r.div_all = r.div_in_burgers = false;
    const bool literal_forcing = !(r.div_all || r.div_in_burgers);      // (the fused forcing launches may decline: the literal sums serve then)
    const bool per_equation = burgers && !(r.div_all || r.batched);
    double *txc[9] = {p, tmp1, literal_forcing ? pressure_work(d, PW_TMP3) : nullptr, tmp2, r.stag ? pressure_work(d, PW_TMP5) : nullptr, nullptr,
                      per_equation ? pressure_work(d, PW_TMP7) : nullptr, per_equation ? pressure_work(d, PW_TMP8) : nullptr,
                      per_equation ? pressure_work(d, PW_TMP9) : nullptr};
    const Ctx c(d, 1.0, q, s, tmp, nullptr, txc, nullptr, true);
    const size_t bytes = (size_t)c.n * sizeof(double);
    if (dcmp == TLAB_DCMP_DIFFUSION || dcmp == TLAB_DCMP_ADVECTION) {
        // the Burgers launches with an all-zero advecting velocity (tmp9 = 0, :117): into the sums themselves (diffusion), or into tmp[3..5], which
        // are then taken from the sums of the first pass (advection = advdiff - diffusion, :145-148)
        hk(hipMemsetAsync(tmp[6], 0, bytes, c.st), "memset");
        double *const zero[3] = {tmp[6], tmp[6], tmp[6]};
        if (dcmp == TLAB_DCMP_ADVECTION) burgers_sums(c, r, equations(c, false), true);
        const Ctx cd(d, 1.0, q, s, dcmp == TLAB_DCMP_ADVECTION ? tmp + 3 : tmp, nullptr, txc, nullptr, true, zero);
        burgers_sums(cd, r, equations(cd, false), true);
        if (dcmp == TLAB_DCMP_ADVECTION) hk(launch_sub3(tmp[0], tmp[1], tmp[2], tmp[3], tmp[4], tmp[5], c.n, c.st), "sub3");
    } else if (burgers) {
        burgers_sums(c, r, equations(c, false), true);      // (total: the body forces in the mid-sequence slot, r.forces)
    } else {
        // Rotation_Coriolis (:158-163) or the buoyancy (:166-196) alone on zeroed sums: one launch of k_body_force with the other term switched off
        // in a copy of the driver's forces
        for (int i = 0; i < 3; ++i) hk(hipMemsetAsync(tmp[i], 0, bytes, c.st), "memset");
        tlab::BodyForce F = d->force;
        if (dcmp == TLAB_DCMP_CORIOLIS) F.bod = 0;
        else F.cor = 0;
        hk(launch_body_force(F, tmp, q, s, d->bprof, c.nx, c.ny, c.nz, c.st), "body force");
    }
    pressure_forcing(c, r);
    pressure_solve(c, r);
    if (r.stag) {      // back onto the velocity nodes (:272-275)
        ok(tlab_opr_partial(3, c.gz, TLAB_OPR_P0_INT_PV, c.nx, c.ny, c.nz, B0, p, c.tmp5, nullptr), "OPR_Partial_Z(P0_INT_PV)");
        ok(tlab_opr_partial(1, c.gx, TLAB_OPR_P0_INT_PV, c.nx, c.ny, c.nz, B0, c.tmp5, p, nullptr), "OPR_Partial_X(P0_INT_PV)");
    }
}

extern "C" {

int tlab_dns_pressure(tlab_dns_t d, int decomposition, double *const *q, double *const *s, double *p, double *tmp1, double *tmp2, double *const *tmp,
                      int ntmp) {
    (void)tlab_internal_deferred_flush();
    return catch_fail([&] {      // (the arguments are checked first: a refusal needs no device)
        const char *who = "tlab_dns_pressure";
        const int dc = decomposition;
        if (dc != TLAB_DCMP_TOTAL && dc != TLAB_DCMP_ADVECTION && dc != TLAB_DCMP_ADVDIFF && dc != TLAB_DCMP_DIFFUSION && dc != TLAB_DCMP_CORIOLIS &&
            dc != TLAB_DCMP_BUOYANCY)
            throw Fail(TLAB_EINVAL, std::string(who) + ": decomposition must be DCMP_TOTAL, _ADVECTION, _ADVDIFF, _DIFFUSION, _CORIOLIS or _BUOYANCY");
        const int need = dc == TLAB_DCMP_ADVECTION || dc == TLAB_DCMP_DIFFUSION ? 7 : 3;
        if (ntmp < need) throw Fail(TLAB_EINVAL, std::string(who) + ": this decomposition needs " + std::to_string(need) + " work arrays in tmp");
        if (!d || !q || !p || !tmp1 || !tmp2 || !tmp || (d->nscal > 0 && !s)) throw Fail(TLAB_EINVAL, std::string(who) + ": a null pointer");
        for (int i = 0; i < 3; ++i)
            if (!q[i]) throw Fail(TLAB_EINVAL, std::string(who) + ": a null velocity array");
        for (int i = 0; i < need; ++i)
            if (!tmp[i]) throw Fail(TLAB_EINVAL, std::string(who) + ": a null work array");
        if (!tlab_device_ready()) throw Fail(TLAB_EHIP, "tlab_init has not been called (no CPU fallback exists)");
        pressure_boussinesq(d, dc, q, s, p, tmp1, tmp2, tmp);
    }, TLAB_EINVAL);
}

int tlab_rhs_global_incompressible_1(tlab_dns_t d, double dte, double *const *q, double *const *s, double *const *hq,
                                     double *const *hs, double *const *txc) {
    return catch_fail([&] {
        if (!d || !q || !hq || !txc || (d->nscal > 0 && (!s || !hs)) || dte <= 0.0) throw Fail(TLAB_EINVAL, "tlab_rhs_global_incompressible_1: bad arguments");
        rhs_substep(d, dte, q, s, hq, hs, txc, nullptr);
    }, TLAB_EINVAL);
}

void tlab_internal_dns_substep(tlab_dns_t d, double dte, double *const *q, double *const *s, double *const *hq, double *const *hs, double *const *txc,
                               const SubstepTail &tail) {
    // the reference computes the liquid from the unclipped scalars and clips afterwards (time.f90:248-250); the epilogues here clip first
    if (d->mixture != TLAB_MIXT_NONE && tail.bounds && tail.bounds->any())
        throw Fail(TLAB_EUNSUPPORTED, "a mixture (diagnostic liquid) together with active scalar bounds: FI_DIAGNOSTIC would see the clipped scalars, the reference's sees the unclipped ones");
    rhs_substep(d, dte, q, s, hq, hs, txc, &tail);
    diagnostic(d, s, tlab_current_stream());      // FI_DIAGNOSTIC after s += dte hs (time.f90:248)
}

int tlab_time_substep_incompressible_explicit(tlab_dns_t d, double dte, double kco, int scale_tendencies, double *const *q,
                                              double *const *s, double *const *hq, double *const *hs, double *const *txc) {
    return catch_fail([&] {
        if (!d || !q || !hq || !txc || (d->nscal > 0 && (!s || !hs)) || dte <= 0.0) throw Fail(TLAB_EINVAL, "tlab_time_substep_incompressible_explicit: bad arguments");
        tlab_internal_dns_substep(d, dte, q, s, hq, hs, txc, {kco, scale_tendencies, &d->bounds, true, true, true});
    }, TLAB_EINVAL);
}

}  // extern "C"

// The single-domain driver's state (struct tlab_dns behind tlab_dns_t) and what the files that work on it call in each other.  Private to the
// library: dns_setup.cpp creates, configures and destroys the driver, rhs.cpp runs its substep, dns_monitors.cpp its monitors, placement.cpp times
// its substep on candidate allocations.  The helpers below are not exported (TLAB_HIDDEN); what OTHER parts of the library call is in internal.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "driver_common.hpp"
#include "kernels.hpp"
#include "plan.hpp"

#define TLAB_HIDDEN __attribute__((visibility("hidden")))

struct tlab_dns {
    tlab_fdm_plan_t g[3];
    tlab_poisson_plan_t poisson;
    int nx, ny, nz, nscal;
    double visc;
    std::vector<double> schmidt;
    double *bcs_hb = nullptr, *bcs_ht = nullptr;   // BcsFlowJmin%ref(:,:,2), BcsFlowJmax%ref(:,:,2)
    bool fuse = true;                              // fold the pointwise sums into the operator kernels where the fast kernels apply
    tlab_filter_t pfilter[3] = {nullptr, nullptr, nullptr};      // PressureFilter(1:3) (not owned) and its repeat counts
    int pfilter_rep[3] = {1, 1, 1};
    tlab_filter_t dfilter[3] = {nullptr, nullptr, nullptr};      // FilterDomain(1:3) of DNS_FILTER (not owned) and its repeat counts (tlab_dns_set_filter)
    int dfilter_rep[3] = {1, 1, 1};
    bool stagger = false;                          // [Staggering] StaggerHorizontalPressure: taken from the x / z plans at creation (tlab_fdm_plan_set_stagger)
    bool remove_divergence = true;                 // [Main] ... forcing = div(hq + q/dte) (rhs_global_incompressible_1.f90:177-232); false: div(hq) (:234-250)
    bool fresh = false;                            // one-shot: hq, hs count as zero on entry of the next substep (tlab_dns_begin_step)
    tlab::WallBcs bcs;
    tlab::ScalarBounds bounds;                           // [Control] ScalLimit
    // dynamic surface model of the scalars (BcsScalJmin/Jmax%SfcType = DNS_SFC_LINEAR, %cpl; boundary_bcs.f90:29-31, 49-50, 478-546)
    std::vector<int> sfc_jmin, sfc_jmax;
    std::vector<double> cpl_jmin, cpl_jmax;
    std::vector<double *> sref_b, sref_t;          // BcsScalJmin%ref(:,:,is), BcsScalJmax%ref(:,:,is) of the scalars with a surface model
    double *sfc_avg = nullptr;                     // one double: plane average
    // TIME_COURANT (tools/dns/time.f90:138-176): ds(ig)%one_ov_ds1 = 1/jac(:,1) on the device, dx2i, schmidtfactor
    double *od[3] = {nullptr, nullptr, nullptr};
    double *part = nullptr;                        // [2][NPART] partial (min, max) of the reductions
    double dx2i = 0.0, schmidtfactor = 0.0;
    int koffset = 0, nz_total = 0;                 // z-slab: first global plane and global nz (one_ov_ds1 of z is indexed globally)
    // nse_eqns == DNS_EQNS_ANELASTIC: rbackground, ribackground (ny values each) on the device; the wall values of rbackground on the host
    double *rb = nullptr, *rib = nullptr;
    // BOUNDARY_BCS_NEUMANN_Y as a weighted sum over the rows next to the wall (neumann_weights below): per variant ibc = 1..3 the device weights
    // [2][K] (bottom, top), K, and six scratch planes
    struct NeuW { double *w = nullptr; int K = 0; bool tried = false; } neuw[4];
    double *wall_planes = nullptr;
    double rb_wall[2] = {1.0, 1.0};
    // [BufferZone] Type = relaxation: BuffFlowJmin/Jmax, BuffScalJmin/Jmax (boundary_buffer.f90) -- buff[group][end], group 0 flow / 1 scalars,
    // end 0 Jmin / 1 Jmax; size 0: that block is off.  tau (size, nf) and ref (nx, size, nz, nf) are device memory the driver owns.
    struct BufferBlock { int size = 0, offset = 0, nf = 0; double *tau = nullptr, *ref = nullptr; } buff[2][2];
    // [Rotation] and [BodyForce] (tlab_dns_set_coriolis / _set_buoyancy): TLab_Sources_Flow as the one launch of k_body_force; bprof: the ny values
    // the buoyancy function subtracts (or starts from), made from bbackground when it is set
    tlab::BodyForce force;
    double *bprof = nullptr;
    bool bback = false;                            // a non-zero bbackground went into bprof (DCMP_BUOYANCY of the pressure subtracts it for y alone)
    // tlab_dns_pressure (FI_PRESSURE_BOUSSINESQ): the work arrays of a route beyond what the caller hands, isize_txc_field doubles each, made on first use
    double *pwork[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    // [Thermodynamics] Mixture (tlab_dns_set_mixture): with one set, s carries inb_scal_array = nscal + 1 arrays, the last the diagnostic liquid
    int mixture = TLAB_MIXT_NONE;
    std::vector<double> thermo_param;
    // [Infrared] (tlab_dns_set_infrared): the gray-liquid heating of TLab_Sources_Scal on scalar ir.scalar (1-based); tab: the shared coefficients of
    // the lambda = 0 integral system of the y plan on the device, built when the term is first switched on
    struct Infrared { int type = TLAB_IR_NONE, scalar = 0; double kappa = 0.0, flux_top = 0.0, flux_bottom = 0.0; double *tab = nullptr; tlab::InfraredCoef C{}; } ir;
    // [Particles] (tlab_dns_set_particles): made and read by particles.hip, null without particles; no launch of the flow substep depends on it
    tlab::ParticleState *particles = nullptr;
    // tlab_dns_arm_pressure_sampling: one-shot, taken by the next substep between the pressure solve and the pressure gradient (the towers' and the
    // phase averages' tap of rhs_global_incompressible_1.f90:292-305).  Nothing is owned: the tower plan and the accumulators are the caller's.
    struct PressureSampling {
        bool armed = false;
        tlab_tower_t tower = nullptr;
        double *tower_buf = nullptr, *phase_avg = nullptr;
        int itime = 0, avg_planes = 0, plane_id = 0;
        double rtime = 0.0;
    } psample;
    int scal_arrays() const { return nscal + (mixture != TLAB_MIXT_NONE ? 1 : 0); }
    TLAB_HIDDEN bool pressure_filter_set() const { return pfilter[0] || pfilter[1] || pfilter[2]; }
    TLAB_HIDDEN bool surface(int is) const { return !sfc_jmin.empty() && (sfc_jmin[is] == 1 || sfc_jmax[is] == 1); }      // scalar is has a surface model at one end
    TLAB_HIDDEN bool buffer_any(int group) const { return buff[group][0].size > 0 || buff[group][1].size > 0; }
    TLAB_HIDDEN bool infrared_on() const { return ir.type == TLAB_IR_GRAY_LIQUID && mixture != TLAB_MIXT_NONE; }
    unsigned long anel_version = 0;                // change counter of the operator state these mirror (follow_anelastic)
    bool anel_owner = false;                       // this driver switched the operator state on (tlab_dns_set_anelastic): it goes with the driver
    ~tlab_dns() {
        if (bcs_hb) (void)hipFree(bcs_hb);
        if (bcs_ht) (void)hipFree(bcs_ht);
        for (int i = 0; i < 3; ++i)
            if (od[i]) (void)hipFree(od[i]);
        if (part) (void)hipFree(part);
        for (double *p : sref_b) if (p) (void)hipFree(p);
        for (double *p : sref_t) if (p) (void)hipFree(p);
        if (sfc_avg) (void)hipFree(sfc_avg);
        if (rb) (void)hipFree(rb);
        if (rib) (void)hipFree(rib);
        for (NeuW &n : neuw) if (n.w) (void)hipFree(n.w);
        if (wall_planes) (void)hipFree(wall_planes);
        if (bprof) (void)hipFree(bprof);
        for (double *p : pwork) if (p) (void)hipFree(p);
        if (ir.tab) (void)hipFree(ir.tab);
        tlab_internal_particles_free(particles);
        for (auto &g : buff)
            for (BufferBlock &b : g) free_block(b, false);
    }
    // the tables of a block go back; sync: kernels that read them may still be in flight on the library's stream
    static void free_block(BufferBlock &b, bool sync) {
        if (sync && (b.tau || b.ref)) (void)hipStreamSynchronize(tlab_current_stream());
        if (b.tau) (void)hipFree(b.tau);
        if (b.ref) (void)hipFree(b.ref);
        b = BufferBlock();
    }
};

namespace tlab {
// ---- rhs.cpp ----
// The wall-plane weights of the Neumann variant ibc = 1..3 (d->neuw[ibc]), built and cached on first use: allocations, launches on the library's
// stream and a synchronisation.  false: not available (the derivative pass serves).  tlab_dns_set_bcs builds those of the variants in use.
TLAB_HIDDEN bool neumann_weights(tlab_dns *d, int ibc);
// the driver's density weights follow the anelastic state of the operators (tlab_opr_burgers_set_anelastic), whichever entry point set it
TLAB_HIDDEN void follow_anelastic(tlab_dns *d);
// the launches of one substep; tail: what follows the RHS (SubstepTail), NULL: the RHS on its own -- no update, no scalar zones, no forces
TLAB_HIDDEN void rhs_substep(tlab_dns *d, double dte, double *const *q, double *const *s, double *const *hq, double *const *hs, double *const *txc,
                             const SubstepTail *tail);
// FI_PRESSURE_BOUSSINESQ: the Burgers, forcing and solve stages of that substep on the sums tmp[0..2] (tmp[0..6] for DCMP_ADVECTION and _DIFFUSION)
// with p as the forcing array; dcmp: a checked TLAB_DCMP_*.  No driver state changes but the scratch d->pwork and the solver's two wall planes.
TLAB_HIDDEN void pressure_boussinesq(tlab_dns *d, int dcmp, double *const *q, double *const *s, double *p, double *tmp1, double *tmp2,
                                     double *const *tmp);

// ---- sampling.cpp ----
// the samples of an armed substep: DNS_TOWER_ACCUMULATE(p, 4) and / or AvgPhaseSpace of p, p the pressure on the velocity nodes (device memory)
TLAB_HIDDEN void pressure_sampling(tlab_dns *d, const tlab_dns::PressureSampling &ps, const double *p);

// ---- dns_setup.cpp: the launches the substep shares with the entry points tlab_dns_buffer_relax_* / _sources_* / _diagnostic ----
// RELAX_BLOCK of the blocks of one group (0: BOUNDARY_BUFFER_RELAX_FLOW on q, hq; 1: BOUNDARY_BUFFER_RELAX_SCAL on s, hs), Jmin before Jmax, four fields a launch
TLAB_HIDDEN void buffer_relax(tlab_dns *d, int group, double *const *a, double *const *h, hipStream_t st);
// TLab_Sources_Flow (tlab_sources.f90:36-92) on (q, s, hq): Rotation_Coriolis, then hq_i += g_i b, one launch
TLAB_HIDDEN void body_force(tlab_dns *d, double *const *q, double *const *s, double *const *hq, hipStream_t st);
// FI_DIAGNOSTIC (physics/fi_diagnostic.f90:44-47), linear thermodynamics: the liquid s[nscal] from the prognostic scalars
TLAB_HIDDEN void diagnostic(tlab_dns *d, double *const *s, hipStream_t st);
// TLab_Sources_Scal (tlab_sources.f90:152-168) on (s, hs): the infrared heating of the liquid s[nscal] added to hs[scalar-1]; scr1, scr2: scratch fields
TLAB_HIDDEN void sources_scal(tlab_dns *d, double *const *s, double *const *hs, double *scr1, double *scr2, hipStream_t st);
}  // namespace tlab

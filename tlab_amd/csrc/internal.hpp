// What the translation units of libtlab_amd.so call in each other and include/tlab_amd.h does not declare: every such function is declared HERE and
// nowhere else.  The defining file includes this header too, so the compiler holds each definition against the one declaration the callers see
// (the library is linked with -z defs: a call without a definition fails the build).  Grouped by defining file.  What the files of the Poisson solver
// (poisson*.hip) call in each other, with their plan object, is declared in poisson_plan.hpp instead.
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/tlab_amd.h"

namespace tlab {
struct SubstepTail;      // driver_common.hpp
struct ParticleState;    // particles.hip
}

// ---- runtime.cpp ----
// hooks for the other translation units (also libtlab_amd_comm.so: comm.hip)
hipStream_t tlab_current_stream();      // the library's stream; a recorded substep (deferred.cpp) runs first
void tlab_set_error(const std::string &s);
bool tlab_device_ready();

// ---- fdm_plan.cpp ----
// coefficients of BOUNDARY_BCS_NEUMANN_Y (boundary_bcs.f90:368-473): wall value = (u(2) cb0 + u(3) cb1) + u(4) cb2 + cb3 du(2), likewise at the top
void tlab_internal_neumann_y_coefficients(tlab_fdm_plan_t g, int ibc, int ny, double (&cb)[4], double (&ct)[4]);

// ---- operators.cpp ----
// chunks per x line of the wave-per-line kernel for this plan (0: not on that kernel): tlab_fdm_plan_info
int xline_chunks(int n, tlab_fdm_plan_t g);
void tlab_internal_operators_release();      // tlab_finalize
// internal fused variants for the RHS driver; return false when the sizes are not on a fused fast path
// result (+)= d/dx_dir (u + scale*ub)
bool tlab_internal_partial_p1_fusable(int dir, tlab_fdm_plan_t g, int nx, int ny, int nz);
bool tlab_internal_partial_p1_fused(int dir, tlab_fdm_plan_t g, int nx, int ny, int nz, int ibc, const double *u, const double *ub,
                                    double scale, double *result, bool acc);
// result -= d/dx_dir u  (fused kernels only; the caller falls back to OPR_Partial + a subtraction otherwise)
bool tlab_internal_partial_p1_sub(int dir, tlab_fdm_plan_t g, int nx, int ny, int nz, const double *u, double *result);
// The last pass over a field with Neumann walls (ibc: 1 jmin, 2 jmax, 3 both; the other side Dirichlet): BOUNDARY_BCS_NEUMANN_Y on the finished
// tendency h, its wall planes, q += dte h, h *= kco -- one launch along y instead of OPR_Partial_Y + k_neumann_planes + k_final_update.
bool tlab_internal_neumann_final_ok(tlab_fdm_plan_t g, int nx, int ny, int nz);
bool tlab_internal_neumann_final(tlab_fdm_plan_t g, int nx, int ny, int nz, int ibc, double *h, double *q, double dte, double kco, int scale);
// Dirichlet walls only (the tendency is zero on the wall planes); dir = 1 or 3.
// pb, pt (device, [nx][nz]; NULL: zero): the tendencies of the wall planes j = 0 / ny-1 (BOUNDARY_BCS_NEUMANN_Y's values for a Neumann wall)
bool tlab_internal_gradient_final(int dir, tlab_fdm_plan_t g, int nx, int ny, int nz, const double *p, double *q, double *h, double dte,
                                  double kco, int scale, const double *pb = nullptr, const double *pt = nullptr);
// result += nu d2s - vel ds   (only when the fully fused Burgers kernels apply)
bool tlab_internal_burgers_acc(int dir, tlab_fdm_plan_t g, int nx, int ny, int nz, int ibc, double nu, const double *s, const double *vel,
                               double *result);
bool tlab_internal_burgers_fusable(int dir, tlab_fdm_plan_t g, int nx, int ny, int nz);
// ... with the anelastic diffusion weight (tlab_internal_burgers_acc_n's ari): it exists in the wave-per-line kernel and in the 32-line tile form of k_htile
bool tlab_internal_burgers_fusable_anelastic(int dir, tlab_fdm_plan_t g, int nx, int ny, int nz);
// x lines of at most 512 points on the wave-per-line kernel: the launch can finish the substep of a transported field in its epilogue
bool tlab_internal_burgers_can_finish(int dir, tlab_fdm_plan_t g, int nx, int ny, int nz);
// the y / z tile kernel can add its direction's term of the pressure forcing in the epilogue of a one-field launch (RTileArgs::fdiv)
bool tlab_internal_burgers_can_div(int dir, tlab_fdm_plan_t g, int nx, int ny, int nz);
// several transported fields, one advecting velocity: result[f] += nu[f] d2 s[f] - vel d s[f]
bool tlab_internal_burgers_acc_n(int dir, tlab_fdm_plan_t g, int nx, int ny, int nz, int ibc, int nf, const double *nu, const double *const *s,
                                 const double *vel, double *const *result, bool overwrite, const int *finish, double dte, double kco, int scale,
                                 double *divx, double idte, unsigned fresh_mask = 0, const double *ari = nullptr, const int *clip = nullptr,
                                 const double *clip_lo = nullptr, const double *clip_hi = nullptr);
extern "C" {
// the operator state set by tlab_opr_burgers_set_anelastic / _set_dealiasing
bool tlab_internal_anelastic();
// ny of the profiles (0: incompressible), the host copies and the change counter
int tlab_internal_anelastic_state(const double **rb, const double **rib, unsigned long *version);
bool tlab_internal_dealiasing();
// a filter that is being destroyed while still set as Dealiasing(dir) is taken out (tlab_filter_destroy): no dangling pointer in the Burgers operators
void tlab_internal_dealiasing_forget(tlab_filter_t f);
}

// ---- deferred.cpp ----
// a recorded Runge-Kutta tail runs before anything else is enqueued, and before a driver's state changes under it (no-op unless tlab_deferred_enable)
int tlab_internal_deferred_flush();
int tlab_internal_deferred_take_error();      // tlab_sync

// ---- filter.hip ----
void tlab_internal_filter_1d(int dir, tlab_filter_t f, int nx, int ny, int nz, const double *u, double *result, hipStream_t st);

// ---- filter_stream.hip ----
// OPR_FILTER's directional branch on nf device fields in place (x, y, z in that order, each repeat[d] times; repeat NULL: once) with the streaming
// kernels.  Every refusal (tlab::Fail: size mismatch, Repeat < 1, null field) comes before the first launch.
void tlab_internal_filter_fields(int nx, int ny, int nz, tlab_filter_t const *f, const int *repeat, int nf, double *const *u, hipStream_t st,
                                 const char *who);

// ---- poisson.hip ----
bool tlab_internal_poisson_has_own_x(tlab_poisson_plan_t P);
// spectra.cpp: n = (nx, ny, nz) of a single-device plan whose x and z transforms cover the whole box; false for a slab, pencil or nz = 1 plan's layout
bool tlab_internal_poisson_box(tlab_poisson_plan_t P, int *n);
// hooks of the RHS driver (rhs.cpp)
bool tlab_internal_poisson_can_v_final(tlab_poisson_plan_t P);
void tlab_internal_poisson_arm_v_final(tlab_poisson_plan_t P, double *q, double *h, double dte, double kco, int scale);

// ---- zslab.hip ----
// the z-slab operators with the neighbours' halo planes of every operand in buffers of their own ({lo, hi}, 3 planes each)
int tlab_internal_zslab_partial_z(tlab_zslab_plan_t P, int phase, int nx, int ny, const double *u, const double *const *u_halo, const double *ub,
                                  const double *const *ub_halo, double scale, double *head, double *tail, const double *tail_left,
                                  const double *head_right, double *result, int acc);
int tlab_internal_zslab_burgers_z_n(tlab_zslab_plan_t P, int phase, int nx, int ny, int nf, const double *nu, const double *const *s,
                                    const double *const *s_lo, const double *const *s_hi, const double *vel, double *head, double *tail,
                                    const double *tail_left, const double *head_right, double *const *result, int acc, const int *fin, double dte,
                                    double kco, int scale);
int tlab_internal_zslab_gradient_final_z(tlab_zslab_plan_t P, int nx, int ny, const double *p, const double *const *p_halo, const double *tail_left,
                                         const double *head_right, double *q, double *h, double dte, double kco, int scale);

// ---- dns_setup.cpp: the single-domain driver apart from its substep (its state: dns_state.hpp) ----
long long tlab_internal_dns_points(tlab_dns_t d);      // deferred.cpp
int tlab_internal_dns_nscal(tlab_dns_t d);
tlab_poisson_plan_t tlab_internal_dns_poisson(tlab_dns_t d);      // spectra.cpp: the plan whose transforms the driver's statistics use
int tlab_internal_dns_scal_arrays(tlab_dns_t d);      // inb_scal_array: nscal, + 1 (the liquid) with a mixture -- the arrays every s of the entry points holds
// what the driver holds (deferred.cpp; slab.cpp, pencil.cpp: the zones and forces of a rank live in its single-domain handle)
bool tlab_internal_dns_has_bounds(tlab_dns_t d);
bool tlab_internal_dns_has_flow_zones(tlab_dns_t d);
bool tlab_internal_dns_has_scal_zones(tlab_dns_t d);
bool tlab_internal_dns_has_forces(tlab_dns_t d);
// shared by the three drivers: n entries (<= nscal) of active / lo / hi checked, the bounds of the active ones returned (on[is] = 0 otherwise)
bool tlab_internal_check_bounds(const char *who, int nscal, int n, const int *active, const double *lo, const double *hi, std::vector<char> &on,
                                std::vector<double> &blo, std::vector<double> &bhi);
extern "C" {
// the wall-plane weights of a Neumann variant for the other drivers of the library (slab.cpp): 1 and (w = [2][K] device weights, K) when available
int tlab_internal_dns_neumann_weights(tlab_dns_t d, int ibc, const double **w, int *K);
}

// particles.hip: the box, the plans and the equations of a driver, and the slot in which the driver keeps the particle state particles.hip makes
// (the driver frees it through tlab_internal_particles_free); throws tlab::Fail where the anelastic profiles of the operators do not fit the driver
struct tlab_dns_grid {
    int nx, ny, nz;
    tlab_fdm_plan_t g[3];
    bool anelastic;
    tlab::ParticleState **particles;
};
void tlab_internal_dns_grid(tlab_dns_t d, tlab_dns_grid *out);

// ---- pointwise.hip ----
// q += dte h, q = min(max(q, lo), hi), h *= kco: the scalar update of the decomposed drivers with their bounds (pencil.cpp)
int tlab_internal_pw_rk_update_clip(double *q, double *h, double dte, double kco, int scale, long long n, double lo, double hi);

// ---- rhs.cpp ----
extern "C" {
// the substep with the tail the caller hands over (driver_common.hpp: SubstepTail), behind tlab_time_substep_incompressible_explicit -- which passes
// the driver's own settings -- and the replay of a record (deferred.cpp); throws tlab::Fail
void tlab_internal_dns_substep(tlab_dns_t d, double dte, double *const *q, double *const *s, double *const *hq, double *const *hs, double *const *txc,
                               const tlab::SubstepTail &tail);
}

// ---- dns_monitors.cpp ----
extern "C" {
// the TIME_COURANT maximum of a box (nx, ny, nz) at global offsets (ioff, koff), with this driver's tables (the decomposed drivers' monitors)
int tlab_internal_dns_courant(tlab_dns_t d, const double *u, const double *v, const double *w, int nx, int ny, int nz, int ioff, int koff,
                              double *pmax);
}

// ---- particles.hip ----
void tlab_internal_particles_free(tlab::ParticleState *p);

// ---- slab.cpp, pencil.cpp ----
// deferred.cpp: the arrays a decomposed driver is bound to (the ONE local rank of a Fortran / MPI host) and whether it holds scalar bounds of its own
// (tlab_*_set_scalar_bounds); false: not bound, or several local ranks -- loopback runs -- which have no single DAXPY partner
struct tlab_bound_fields {
    double *const *q, *const *s, *const *hq, *const *hs;
    int nscal;
    long long n;
    bool has_bounds;
};
bool tlab_internal_slab_bound(tlab_slab_dns_t d, tlab_bound_fields *out);
bool tlab_internal_pencil_bound(tlab_pencil_dns_t d, tlab_bound_fields *out);
// the substep with the tail the caller hands over, behind tlab_slab_dns_substep / tlab_pencil_dns_substep and the replay of a record; throw tlab::Fail
void tlab_internal_slab_substep(tlab_slab_dns_t d, double dte, const tlab::SubstepTail &tail);
void tlab_internal_pencil_substep(tlab_pencil_dns_t d, double dte, const tlab::SubstepTail &tail);

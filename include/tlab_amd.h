/* tlab_amd.h -- C ABI of the MI355X-native Tlab Navier-Stokes RHS operators.
 *
 * This is the drop-in boundary.  Tlab has no FFI: its boundary is Fortran module procedures
 * (SURVEY.md 8b).  Each entry point below is what an ISO_C_BINDING interface in the same-named
 * Fortran module binds to (tlab_amd/fortran/); the reference interface it replaces
 * is cited as path:line relative to the reference's src/.
 *
 * Conventions
 *  - every function returns 0 on success, a negative TLAB_E* code otherwise; tlab_last_error() gives text.
 *    (reference: operators stop the program through TLab_Stop, base/tlab_workflow.f90:105; the Fortran shim
 *    maps non-zero to TLab_Write_ASCII(efile, ...) + TLab_Stop(DNS_ERROR_UNDEVELOP).)
 *  - all field pointers are DEVICE pointers (hipMalloc / tlab_malloc / torch CUDA tensors), fp64,
 *    x fastest: index = i + nx*(j + ny*k), exactly the host layout of the reference
 *    (operators/opr_partial.f90:40: u(nx*ny*nz)).
 *  - coefficient tables passed IN from a host (tlab_fdm_plan_create_from_arrays) are HOST pointers,
 *    column-major as Fortran stores lhs(n,ndl), rhs(n,ndr).
 *  - kernels are enqueued on the stream set by tlab_set_stream (default: the null stream); nothing
 *    synchronises except tlab_sync() and the *_get / memcpy helpers.
 *  - one in-flight operator per process, like the reference (module state).
 */
#ifndef TLAB_AMD_H
#define TLAB_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- error codes ------------------------------------------------------------------------- */
#define TLAB_OK 0
#define TLAB_EINVAL (-1)      /* bad argument (size, direction, type, aliasing)                  */
#define TLAB_EUNSUPPORTED (-2)/* valid in the reference, not built here (falls to CPU in Fortran) */
#define TLAB_EHIP (-3)        /* HIP / rocFFT / RCCL runtime error                               */
#define TLAB_ENOMEM (-4)

/* ---- constants mirrored from the reference ------------------------------------------------ */
/* operators/opr_partial.f90:19-26 */
#define TLAB_OPR_P1 1
#define TLAB_OPR_P2 2
#define TLAB_OPR_P2_P1 3
#define TLAB_OPR_P1_INT_VP 5   /* interpolatory first derivative velocity -> pressure grid (staggering; periodic x, z) */
#define TLAB_OPR_P1_INT_PV 6
#define TLAB_OPR_P0_INT_VP 7   /* interpolation velocity -> pressure grid */
#define TLAB_OPR_P0_INT_PV 8
/* physics/opr_burgers.f90:29-30 */
#define TLAB_OPR_B_SELF 0
#define TLAB_OPR_B_U_IN 1
/* base/tlab_constants.f90:63-66 */
#define TLAB_BCS_DD 0
#define TLAB_BCS_ND 1
#define TLAB_BCS_DN 2
#define TLAB_BCS_NN 3
/* fdm/fdm_derivative.f90:51-58 */
#define TLAB_FDM_COM4_JACOBIAN 4
#define TLAB_FDM_COM6_JACOBIAN_PENTA 5
#define TLAB_FDM_COM6_JACOBIAN 6
#define TLAB_FDM_COM6_JACOBIAN_HYPER 7

/* ---- runtime ------------------------------------------------------------------------------ */
int tlab_init(int device);                 /* hipSetDevice + library state; idempotent            */
int tlab_device_count(void);               /* visible GPUs (hipGetDeviceCount; 0 if none): a multi-rank host selects mod(local rank, count) */
int tlab_finalize(void);
const char *tlab_last_error(void);
int tlab_set_stream(void *hip_stream);     /* hipStream_t; NULL = default stream                  */
int tlab_sync(void);                       /* hipStreamSynchronize on the current stream          */
/* allocation hook: replaces the allocate() inside TLab_Allocate_Real (base/tlab_memory.f90:306-331) so that
 * q, s, txc, wrk3d, hq, hs live in HBM; the Fortran side wraps the pointer with c_f_pointer. */
int tlab_malloc(void **p, size_t bytes);
int tlab_free(void *p);
int tlab_memcpy_h2d(void *dst, const void *src, size_t bytes);
int tlab_memcpy_d2h(void *dst, const void *src, size_t bytes);

/* ---- FDM plans: type(fdm_dt) of fdm/fdm.f90:14-29 + type(fdm_derivative_dt) fdm_derivative.f90:16-29 ---- */
typedef struct tlab_fdm_plan *tlab_fdm_plan_t;

/* Replaces FDM_CreatePlan (fdm/fdm.f90:143-252): Jacobians from the node positions, compact schemes
 * scheme1 (first derivative: TLAB_FDM_COM4_JACOBIAN | TLAB_FDM_COM6_JACOBIAN | TLAB_FDM_COM6_JACOBIAN_PENTA) and scheme2 (second derivative:
 * COM4_JACOBIAN | COM6_JACOBIAN | COM6_JACOBIAN_HYPER), Neumann variants (FDM_Bcs_Neumann, fdm_base.f90:194),
 * factorizations.  nodes: HOST pointer, n doubles.
 * hyper_bc1_ext: value of the out-of-bounds coefficient the reference reads for the C2N6-Hyper wall row
 * (fdm_com2_jacobian.f90:224 with icmax=4; DESIGN.md "reference defects"): pass 0.1 to reproduce the flang-built
 * reference bit for bit, 0.0 for the consistent closure. */
int tlab_fdm_plan_create(tlab_fdm_plan_t *out, int n, const double *nodes, int periodic, int uniform,
                         int scheme1, int scheme2, double hyper_bc1_ext);

/* Same plan from coefficient tables the (unchanged) Fortran host already built in FDM_Initialize:
 * lhs1 = g%der1%lhs(n,1:ndl1), rhs1 = g%der1%rhs(n,1:ndr1), lhs2 = g%der2%lhs(n,1:ndl2),
 * rhs2 = g%der2%rhs(n,1:ndr2+ndl2) (the last ndl2 columns are the Jacobian-correction diagonals,
 * fdm_derivative.f90:356,437-440).  ndl2 must be 3; ndl1 = 3, or 5 with ndr1 = 7 (CompactJacobian6Penta: the library factorizes with
 * PENTADFS2 / PENTADPFS as fdm_derivative.f90:90-119 does; the derivative then runs one line per thread, no chunked fast path). */
int tlab_fdm_plan_create_from_arrays(tlab_fdm_plan_t *out, int n, int periodic, int need_1der,
                                     int ndl1, int ndr1, const double *lhs1, const double *rhs1,
                                     int ndl2, int ndr2, const double *lhs2, const double *rhs2);
/* Remaining members of type(fdm_dt) a host-built plan may carry (any pointer may be NULL): der1%mwn(n), der2%mwn(n) (periodic directions:
 * OPR_Poisson needs der1%mwn of x and z, opr_elliptic.f90:199-203), jac(n,3) (TIME_COURANT, time.f90:148), nodes(n). */
int tlab_fdm_plan_set_aux(tlab_fdm_plan_t plan, const double *mwn1, const double *mwn2, const double *jac, const double *nodes);
/* mode_fdm of the two derivatives of a host-built plan (fdm_derivative.f90:52-58).  FDM_COM6_DIRECT (16) / FDM_COM4_DIRECT (17) as mode2
 * make rhs2 a per-row pentadiagonal operator (MatMul_5d) -- [Main] SpaceOrder2 = CompactDirect6 of examples/Case81-93; the coefficient
 * tables of fdm_comx_direct.f90 are the host's (tlab_fdm_plan_create_from_arrays).  As mode1 (SpaceOrder1 = CompactDirect4 / CompactDirect6,
 * FDM_C1N4_Direct / FDM_C1N6_Direct: 3 / 5 per-row RHS diagonals, MatMul_3d / MatMul_5d with the Neumann-reduced rows of FDM_Bcs_Neumann)
 * in non-periodic directions (periodic ones fall back to the Jacobian schemes, fdm.f90:155-158). */
int tlab_fdm_plan_set_scheme(tlab_fdm_plan_t plan, int mode1, int mode2);
/* [Staggering] StaggerHorizontalPressure = yes (TLab_WorkFlow::stagger_on): FDM_CreatePlan then gives a periodic direction the interpolation
 * tables g%intl (FDM_Interpol_Initialize, fdm/fdm_interpolate.f90:33-96) and replaces g%der1%mwn by the interpolatory modified wavenumbers
 * (fdm.f90:236-248).  mode 1: both (plans of tlab_fdm_plan_create); 2: tables only (host-built plans whose mwn1 already is the host's); 0: off.
 * With it tlab_opr_partial takes the types TLAB_OPR_P0/P1_INT_VP/PV along x and z, a Poisson plan built on such x / z plans has the one singular
 * mode (1,1) (opr_elliptic.f90:144-146) and the RHS driver takes the staggered branch (rhs_global_incompressible_1.f90:216-226, 266-273, 307-317). */
int tlab_fdm_plan_set_stagger(tlab_fdm_plan_t plan, int mode);
int tlab_fdm_plan_destroy(tlab_fdm_plan_t p);

/* read back plan tables (HOST buffer, column-major like the reference) for parity tests. which:
 *  1 der1%lhs(n,5) 2 der1%rhs(n,7) 3 der1%lu(n,5|20) 4 der1%rhs_b(4,0:7) 5 der1%rhs_t(0:4,7) 6 der1%mwn(n)
 *  7 der2%lhs(n,5) 8 der2%rhs(n,12) 9 der2%lu(n,5|3) 10 der2%mwn(n) 11 jac(n,3) 12 intl%lu0i(n,5) 13 intl%lu1i(n,5)
 * returns the number of doubles written (or <0). */
int tlab_fdm_plan_get(tlab_fdm_plan_t p, int which, double *buf, int nbuf);
int tlab_fdm_plan_info(tlab_fdm_plan_t p, int what); /* 0 n, 1 ndl1, 2 ndr1, 3 ndl2, 4 ndr2, 5 need_1der, 6 periodic, 7 staggered; after tlab_init:
                                                        * 8 chunks per x line of the wave-per-line kernel (64 one wave, 128 / 256 two / four waves
                                                        * per line, 0 another kernel), 9 whether all those chunks share one set of tables (1: an
                                                        * exactly uniform grid, scalar loads; 0: per-chunk tables staged in LDS) */

/* ---- operators ----------------------------------------------------------------------------- */
/* OPR_Partial_X/Y/Z(type, nx, ny, nz, bcs, g, u, result, tmp1)   operators/opr_partial.f90:31,266,154
 * dir = 1,2,3.  ibc = bcs(1,1) + 2*bcs(2,1) (opr_partial.f90:91).  type = TLAB_OPR_P1 | P2 | P2_P1.
 * tmp1: first derivative on return for P2_P1; scratch (may be NULL when the plan needs no Jacobian
 * correction) for P2; unused for P1.  u, result, tmp1 must not alias.  2-D guard: a direction of size 1
 * returns zeros (opr_partial.f90:175-177,287-289). */
int tlab_opr_partial(int dir, tlab_fdm_plan_t g, int type, int nx, int ny, int nz, int ibc,
                     const double *u, double *result, double *tmp1);

/* OPR_Burgers_X/Y/Z(ivel, is, nx, ny, nz, bcs, s, u, result, tmp1, u_t)   physics/opr_burgers.f90:190,277,359
 * result = nu * d2s/dx2 - u * ds/dx along dir; nu = visc (is = 0) or visc/schmidt(is)
 * (OPR_Burgers_Initialize, opr_burgers.f90:92-112, folds it into the LU; here it is an argument).
 * ivel = TLAB_OPR_B_SELF: advecting velocity is s itself; TLAB_OPR_B_U_IN: it is u (natural layout).
 * The reference additionally threads a *transposed* copy of the velocity through tmp1/u_t to save CPU
 * transposes (opr_burgers.f90:236-240); the device kernels read u in its natural layout, so u_t is ignored.
 * If write_transposed != 0 and ivel == SELF, tmp1 receives the transposed operand exactly as the
 * reference leaves it (X: (ny*nz, nx); Y with nz > 1: (nz, nx*ny)), bit-exact; otherwise tmp1 is scratch
 * (first derivative). */
int tlab_opr_burgers(int dir, tlab_fdm_plan_t g, int ivel, int nx, int ny, int nz, int ibc, double nu,
                     const double *s, const double *u, double *result, double *tmp1, int write_transposed);
/* The anelastic branch of OPR_Burgers_1D (physics/opr_burgers.f90:504-507) with the module state OPR_Burgers_Initialize sets up for
 * nse_eqns == DNS_EQNS_ANELASTIC (:128-183): the diffusion term is multiplied by ribackground(j) -- rhoinv(1), rhoinv(3) along x and z, the
 * scaled U factors of fdmDiffusion(2) along y (the same product, rounding aside).  HOST pointers, ny values each; ny = 0 or NULL: off.
 * While it is on, tlab_opr_burgers runs the two derivatives unfused and a weighted epilogue. */
int tlab_opr_burgers_set_anelastic(int ny, const double *rbackground, const double *ribackground);

/* ---- 1-D filters: OPR_FILTER_1D (operators/opr_filter.f90:393-460) and the dealiasing branch of OPR_Burgers_1D ----------------------
 * type(filter_dt) as OPR_FILTER_INITIALIZE leaves it (opr_filter.f90:28-41, 236-275): type = DNS_FILTER_COMPACT 1 | _6E 2 | _4E 3 |
 * _COMPACT_CUTOFF 9 (:56-65; tophat 8 and the 3-D spectral / Helmholtz types: TLAB_EUNSUPPORTED), BcsMin / BcsMax = DNS_FILTER_BCS_* of
 * filters/flt_base.f90:5-11, coeffs = f%coeffs(size, inb_filter), HOST pointer, column-major (NULL for explicit6; the generators
 * FLT_C4_RHS_COEFFS / FLT_E4_COEFFS and the LU of the compact forms stay the host's). */
typedef struct tlab_filter *tlab_filter_t;
#define TLAB_FILTER_COMPACT 1
#define TLAB_FILTER_6E 2
#define TLAB_FILTER_4E 3
#define TLAB_FILTER_COMPACT_CUTOFF 9
int tlab_filter_create(tlab_filter_t *out, int type, int size, int periodic, int bcsmin, int bcsmax, int inb_filter, const double *coeffs);
int tlab_filter_destroy(tlab_filter_t f);
/* result = filter(u) along direction dir of a field (nx, ny, nz), out of place: FLT_C4_RHS + TRIDSS / TRIDPSS, FLT_C4[P]_CUTOFF_RHS + PENTADSS2 /
 * PENTADPSS, FLT_E6, FLT_E4 (src/filters/flt_compact.f90, flt_explitic.f90) -- one line per thread, the reference's operation order. */
int tlab_opr_filter_1d(int dir, tlab_filter_t f, int nx, int ny, int nz, const double *u, double *result);
/* OPR_FILTER(nx, ny, nz, f, u, txc) (opr_filter.f90:283-392), directional branch: the x, y, z filters in that order (NULL = none), each repeat[d]
 * times (NULL = once), in place; tmp: one field of scratch.  A filter whose size is not the extent along its direction and a Repeat < 1 are
 * refused (TLAB_EINVAL) before anything is launched: u is as it was. */
int tlab_opr_filter(int nx, int ny, int nz, tlab_filter_t fx, tlab_filter_t fy, tlab_filter_t fz, const int *repeat, double *u, double *tmp);
/* The same branch of OPR_FILTER on nf device fields u[0..nf-1] (HOST array of device pointers) at once, in place and without a tmp: the streaming
 * kernels of csrc/filter_stream.hip.  A line stays with one thread and keeps the reference's operation order, so every word equals
 * tlab_opr_filter's; it is swept as often as its recursion forces -- once for the explicit types, twice for compact (the right-hand side is formed
 * inside the forward sweep from a register window, TRIDPSS's wrk sum with it), twice for compactcutoff, three times for its periodic form -- and
 * x lines are staged through LDS instead of a transposed scratch.  The same refusals as tlab_opr_filter (size mismatch, Repeat < 1, null
 * pointers), before anything is launched: the fields are as they were. */
int tlab_opr_filter_fields(int nx, int ny, int nz, tlab_filter_t fx, tlab_filter_t fy, tlab_filter_t fz, const int *repeat, int nf, double *const *u);
/* [Dealiasing] Dealiasing(dir) of OPR_Burgers (physics/opr_burgers.f90:33, 71, 118-125): while a filter is set for a direction, tlab_opr_burgers
 * along it computes nu d2s - filter(u) filter(ds/dx) (:478-500), unfused; NULL: none.  The filter is not owned. */
int tlab_opr_burgers_set_dealiasing(int dir, tlab_filter_t f);

/* ---- Poisson solver --------------------------------------------------------------------------- */
/* OPR_Elliptic_Initialize (operators/opr_elliptic.f90:86-250, TYPE_FACTORIZE) + OPR_Fourier_Initialize
 * (operators/opr_fourier.f90:54-208): eigenvalues lambda(k,i) from the modified wavenumbers of the x and z plans,
 * singular modes, first-order integral operators of the y plan, rocFFT plans, and the homogeneous solutions of
 * every mode.  Serial decomposition (one GPU owns all of x and z). */
typedef struct tlab_poisson_plan *tlab_poisson_plan_t;
int tlab_poisson_plan_create(tlab_poisson_plan_t *out, tlab_fdm_plan_t gx, tlab_fdm_plan_t gy, tlab_fdm_plan_t gz,
                             int nx, int ny, int nz);
int tlab_poisson_plan_destroy(tlab_poisson_plan_t p);

/* OPR_Poisson(nx, ny, nz, ibc, p, tmp1, tmp2, bcs_hb, bcs_ht, dpdy)   operators/opr_elliptic.f90:33-46, :263-364
 * Solves lap p = f with periodic x, z.  ibc = TLAB_BCS_NN: bcs_hb, bcs_ht (nx*nz each) are dp/dy at the walls (OPR_ODE2_Factorize_NN / _NN_Sing per
 * mode: the call of the RHS); ibc = TLAB_BCS_DD: they are p at the walls (OPR_ODE2_Factorize_DD / _DD_Sing, opr_elliptic.f90:322-329; marching
 * kernels, 2.4x the time of the per-mode stage, work arrays allocated on first use).  The reference has no other type for the factorized solver
 * (:312-331); direct plans (below) take all four.  p: forcing in, solution out (its wall planes are overwritten with the BC
 * data first, like the reference :285-286).  tmp1, tmp2: work arrays of isize_txc_field = (nx+2)*ny*nz doubles
 * (base/tlab_memory.f90:186-187), destroyed.  dpdy (may be NULL): dp/dy. */
int tlab_opr_poisson(tlab_poisson_plan_t plan, int nx, int ny, int nz, int ibc, double *p, double *tmp1, double *tmp2,
                     const double *bcs_hb, const double *bcs_ht, double *dpdy);

/* Which per-mode solver the factorized plans created AFTER this call use (also TLAB_POISSON_EXACT=1 in the environment):
 *   0 (default): k_ode_nn, the register-chunked solver (2.4 ms at 512^3).  Its substitutions run as a parallel scan over 8-row chunks, i.e. in
 *      another order than the reference's serial sweeps: as accurate as the reference, but where the problem amplifies rounding (the
 *      projection of a non-solenoidal field: forcing div(q)/dte ~ 1e4-1e6 for a pressure of 1e2-1e3) the two would differ by what two builds of
 *      the reference itself differ by (with / without fused multiply-adds: 4e-12 in p, 1.4e-11 in dp/dy on 512-point lines; one ulp of
 *      forcing noise -- another FFT library -- gives 6e-13 and 2.5e-12).  That difference sits in the few modes with lambda h^2 << 1, so on a
 *      single device those (at most 128 modes, sqrt(lambda) mean(h) <= 0.06) are solved by a marching sub-plan beside k_ode_nn
 *      (TLAB_POISSON_LOW_MODES=0 turns it off; decomposed plans run it on the rank that owns kx = 0..): 7.6e-13 /
 *      3.1e-12 on that projection, <= 3e-13 / 9e-13 on forcing without the cancellation; costs 0.1-0.2 ms per solve.
 *   1: the marching kernels (k_int1: one thread per mode, 5.8 ms at 512^3), which repeat FDM_Int1_Solve / OPR_ODE2_Factorize_NN operation by
 *      operation, in the reference's order and without fused multiply-adds: 4e-13 / 1.7e-12 on the same case, i.e. at the FFT-noise floor. */
int tlab_poisson_set_exact(int on);

/* EllipticOrder = CompactDirect6: OPR_Elliptic_Initialize with TYPE_DIRECT (operators/opr_elliptic.f90:107-163, 228-245) and
 * OPR_Poisson_FourierXZ_Direct (:368-455).  gy_elliptic is the reference's fdm_loc: a y plan whose second derivative holds the CompactDirect6
 * tables (tlab_fdm_plan_create_from_arrays + tlab_fdm_plan_set_scheme(.., 16) + tlab_fdm_plan_set_aux(.. nodes)); gy stays the plan of the
 * derivatives (dp/dy = OPR_Partial_Y(OPR_P1, p), :447-449; NOT owned, must outlive the Poisson plan).  lambda(k,i) = mwn2_x(i) + mwn2_z(k) from
 * the SECOND-derivative modified wavenumbers of gx, gz; one singular mode (1,1), solved with BCS_DN and p = 0 at the bottom.  Per mode one
 * second-order integral solve (FDM_Int2_Initialize / FDM_Int2_Solve, fdm/fdm_integral.f90:334-673).  With such a plan tlab_opr_poisson accepts
 * ibc = TLAB_BCS_DD / ND / DN / NN (bcs_hb, bcs_ht: function value at a D end, derivative at an N end). */
int tlab_poisson_plan_create_direct(tlab_poisson_plan_t *out, tlab_fdm_plan_t gx, tlab_fdm_plan_t gy, tlab_fdm_plan_t gz,
                                    int nx, int ny, int nz, tlab_fdm_plan_t gy_elliptic);
/* OPR_Helmholtz(nx, ny, nz, ibc, alpha, a, tmp1, tmp2, bcs_hb, bcs_ht)   operators/opr_elliptic.f90:48-62
 * Solves lap a + alpha a = f (the solver of the implicit RK, alpha < 0).  a: forcing in, solution out; tmp1, tmp2 as tlab_opr_poisson.
 * - DIRECT plan: OPR_Helmholtz_FourierXZ_Direct (:562-628), per mode the second-order integral system with constant lambda2 - alpha, any of
 *   the four boundary types, no singular-mode treatment.
 * - factorized plan of tlab_poisson_plan_create: OPR_Helmholtz_FourierXZ_Factorize (:466-557), per mode OPR_ODE2_Factorize_NN / _DD with
 *   sqrt(lambda - alpha) (must be positive for every mode), ibc = TLAB_BCS_NN or TLAB_BCS_DD (others: TLAB_EUNSUPPORTED, like the reference).
 *   Where the reference factorizes 2 systems per mode on every call (:518-522), the tables of an alpha are built on its first call and kept
 *   (the 4 most recent alphas; about 6 field-sized arrays each); the x, y, z plans given to tlab_poisson_plan_create must still be alive. */
int tlab_opr_helmholtz(tlab_poisson_plan_t plan, int nx, int ny, int nz, int ibc, double alpha, double *a, double *tmp1, double *tmp2,
                       const double *bcs_hb, const double *bcs_ht);
/* Decomposed direct plans, driven stage by stage like the factorized ones (set_wall_planes, fft_x, [exchange], fft_z, tlab_poisson_direct_ode,
 * fft_z, [exchange], fft_x) -- with ONE field on the way back: dp/dy is OPR_Partial_Y of p on the slab (y is never split).
 * mode 0: z-slab plan, (a, b) = (koffset, nproc_k) as tlab_poisson_plan_create_slab; mode 1: kx-pencil plan, (a, b) = (ioffset, nxl). */
int tlab_poisson_plan_create_direct_decomposed(tlab_poisson_plan_t *out, tlab_fdm_plan_t gx, tlab_fdm_plan_t gy, tlab_fdm_plan_t gz,
                                               int nx, int ny, int kmax, int nz_total, int mode, int a, int b, tlab_fdm_plan_t gy_elliptic);
/* the per-mode stage of a direct plan on spectral fields (nx/2+1, ny, nz) complex: f_hat -> p_hat (may alias) */
int tlab_poisson_direct_ode(tlab_poisson_plan_t plan, int ibc, double *f_hat, double *p_hat);

/* z-slab variant (ims_npro_k = nproc_k ranks, one GPU each; base/tlab_mpi_procs.f90:76-94): this rank owns planes
 * [koffset, koffset + kmax) of nz_total.  The per-mode tables are built for the rank's own kz range (opr_elliptic.f90:167-194)
 * and the z transform works on the K-transposed layout (nlines = (nx/2+1)*ny/nproc_k lines of nz_total points).  Such a plan is
 * driven stage by stage, with the caller's all-to-all (TLabMPI_Trp_ExecK_*, base/tlab_mpi_transpose.f90:343-458) in between:
 *   set_wall_planes, fft_x(+1), [K-forward], fft_z(+1), [K-backward], ode, [K-forward], fft_z(-1), [K-backward], fft_x(-1).  */
int tlab_poisson_plan_create_slab(tlab_poisson_plan_t *out, tlab_fdm_plan_t gx, tlab_fdm_plan_t gy, tlab_fdm_plan_t gz,
                                  int nx, int ny, int kmax, int nz_total, int koffset, int nproc_k);
/* kx-pencil variant: the physical box is the z-slab (nx, ny, kmax); the spectral box holds the kx range [ioffset, ioffset+nxl) of
 * ALL kz: (nxl, ny, nz_total).  One all-to-all (slab -> pencil) after fft_x(+1) and one before fft_x(-1) replace the four
 * K-transposes per field of the plan above; fft_z and ode then work on the pencil:
 *   set_wall_planes, fft_x(+1), [slab->pencil], fft_z(+1), ode, fft_z(-1), [pencil->slab], fft_x(-1).  */
int tlab_poisson_plan_create_pencil(tlab_poisson_plan_t *out, tlab_fdm_plan_t gx, tlab_fdm_plan_t gy, tlab_fdm_plan_t gz,
                                    int nx, int ny, int kmax, int nz_total, int ioffset, int nxl);
/* Repacking around the slab <-> pencil all-to-all: slab = complex (nxh, ny, kmax); buffer = for every peer p the block [kmax][ny][nxl_p] of
 * its kx range [ioff[p], ioff[p+1]) (ioff[nproc] = nxh implied), blocks back to back.  dir = +1 slab -> buffer, -1 buffer -> slab.  nproc <= 8.
 * (The pencil side needs no repacking: z is its slowest index.)  Bit-exact index work. */
int tlab_pencil_repack(double *slab, double *buffer, int nxh, int ny, int kmax, int nproc, const int *ioff, int dir);
/* The same with up to 16 blocks placed anywhere in the buffer: block b = kx range [start[b], start[b+1]) (the last one ends at nx/2+1), laid out
 * [kmax][ny][width] from complex element base[b] on.  Used by the slab driver to send every peer's kx range in two halves, all first halves
 * ahead of all second halves, so that the solves of one half run while the other half is on the wire (tlab_amd/parallel.py). */
int tlab_pencil_repack_blocks(double *slab, double *buffer, int nxh, int ny, int kmax, int nblocks, const int *start, const long long *base, int dir);
int tlab_poisson_set_wall_planes(tlab_poisson_plan_t plan, double *p, const double *bcs_hb, const double *bcs_ht);
/* OPR_Fourier_X_Forward (dir = +1) / _Backward (dir = -1), opr_fourier.f90:219,277; out of place, unnormalised like FFTW.  The forward transform is
 * the library's one-pass kernel where its lengths apply (nx/2 = 8^a * {1,2,4}, 128 <= nx <= 2048), rocFFT otherwise; the backward one is rocFFT's.
 * dir = -2: the library's own inverse kernel (the one that finishes the v equation inside tlab_opr_poisson when the RHS driver asks for it), for tests. */
int tlab_poisson_fft_x(tlab_poisson_plan_t plan, int dir, double *in, double *out);
/* The same transforms with the complex side directly in the pack layout of tlab_pencil_repack_blocks (same nblocks / start / base), i.e. the
 * repack pass folded into the library's own x-transform kernels: dir = +1 real in -> pack buffer out, dir = -1 pack buffer in -> real out.
 * _final: the inverse of dp^/dy finishes the v equation in its epilogue (h = h - dp/dy, wall planes of h zeroed, q += dte h, h *= kco when
 * scale; rhs_global_incompressible_1.f90:236-241,258-261 + time.f90 RK update) instead of writing dp/dy.  TLAB_EUNSUPPORTED where the own
 * kernels do not apply (see above); the inverse differs from rocFFT's by rounding.  Used by the native slab driver (tlab_slab_dns_*). */
int tlab_poisson_fft_x_packed(tlab_poisson_plan_t plan, int dir, double *in, double *out, int nblocks, const int *start, const long long *base);
int tlab_poisson_fft_x_packed_final(tlab_poisson_plan_t plan, double *in, double *q, double *h, double dte, double kco, int scale, int nblocks,
                                    const int *start, const long long *base);
int tlab_poisson_fft_z(tlab_poisson_plan_t plan, int dir, double *in, double *out);   /* the FFT inside OPR_Fourier_Z_*, :355,422 */
int tlab_poisson_ode(tlab_poisson_plan_t plan, double *f_hat, double *p_hat, double *dp_hat); /* mode loop of opr_elliptic.f90:308-333 */

/* Accumulating forms of the two operators, as the RHS uses them (hq = hq + OPR_Burgers(...), tmp = tmp + OPR_Partial(hq + q/dte)):
 *   tlab_opr_burgers_add : result += nu d2s/dx2 - vel ds/dx                       (rhs_global_incompressible_1.f90:98-136 + :106-112)
 *   tlab_opr_partial_add : result (+)= d/dx (u + scale*ub)   (ub may be NULL; acc = 0 overwrites)        (:197-201, :228-230, :257-259)
 * One fused kernel when the sizes are on a fast path; otherwise the reference's own sequence with the temporaries tmp1, tmp2. */
int tlab_opr_burgers_add(int dir, tlab_fdm_plan_t g, int nx, int ny, int nz, int ibc, double nu, const double *s, const double *vel,
                         double *result, double *tmp1, double *tmp2);
int tlab_opr_partial_add(int dir, tlab_fdm_plan_t g, int nx, int ny, int nz, int ibc, const double *u, const double *ub, double scale,
                         double *result, int acc, double *tmp1, double *tmp2);
/* Last pass over a velocity component folded into the pressure gradient (Dirichlet walls): h -= dp/dx_dir; h = 0 on the wall planes
 * j = 1, ny; q += dte h; h *= kco if scale (rhs_global_incompressible_1.f90:319-320, :348-352, :373-375; time.f90:645-664, :272-297).
 * One kernel on a fast path (dir = 1, 3), otherwise OPR_Partial into tmp1 + the pointwise pass. */
int tlab_opr_gradient_final(int dir, tlab_fdm_plan_t g, int nx, int ny, int nz, const double *p, double *q, double *h, double dte,
                            double kco, int scale, double *tmp1);
/* nf (1..4) transported fields advected by the same velocity (the u-, v-, w- and scalar equations all call OPR_Burgers_X with u, etc.):
 * result[f] += nu[f] d2s[f]/dx2 - vel ds[f]/dx in one launch, the velocity being fetched from HBM once.  HOST arrays of DEVICE pointers.
 * overwrite != 0: result[f] = ... (the tendencies are zero at the start of a Runge-Kutta step, time.f90:212-216: no fill, no read). */
int tlab_opr_burgers_add_n(int dir, tlab_fdm_plan_t g, int nx, int ny, int nz, int ibc, int nf, const double *nu, const double *const *s,
                           const double *vel, double *const *result, double *tmp1, double *tmp2, int overwrite);

/* ---- z-derivatives on a z-slab without transposes (multi-GPU) ---------------------------------------------
 * Replaces TLabMPI_Trp_ExecK_Forward + OPR_Partial_Z / OPR_Burgers_Z + TLabMPI_Trp_ExecK_Backward (opr_partial.f90:154-262,
 * opr_burgers.f90:331-440, base/tlab_mpi_transpose.f90:343-458) for a periodic z split into slabs of kmax planes: the compact
 * system is partitioned at the slab boundaries, so that a slab only needs 3 halo planes of the operand and, per line and
 * implicit system, one value from each neighbour (see tlab_amd/csrc/zslab.hip).  Two-phase protocol per operator:
 *   phase 1: head[nsys][nx*ny], tail[nsys][nx*ny] are written          (nsys = 1 for partial_z, 2 for burgers_z)
 *   caller:  tail -> right neighbour (arrives as tail_left), head -> left neighbour (arrives as head_right)
 *   phase 2: result = d/dz (u [+ scale*ub])   resp.   nu d2s/dz2 - vel ds/dz ;  acc != 0: result += ...
 * Every operand pointer addresses the first plane of the slab and must have 3 valid planes before it and after the slab
 * (the neighbours' planes, periodic in z).  plan_create returns TLAB_EUNSUPPORTED when the slab is too thin for the coupling
 * between slab separators to vanish in double precision (kmax >~ 50 for the sixth-order schemes): keep the transpose path then.
 * chunk: rows per wave (0 = automatic, 16 or 32). */
typedef struct tlab_zslab_plan *tlab_zslab_plan_t;
int tlab_zslab_plan_create(tlab_zslab_plan_t *out, tlab_fdm_plan_t gz, int kmax, int koffset, int chunk);
int tlab_zslab_plan_destroy(tlab_zslab_plan_t plan);
int tlab_zslab_partial_z(tlab_zslab_plan_t plan, int phase, int nx, int ny, const double *u, const double *ub, double scale,
                         double *head, double *tail, const double *tail_left, const double *head_right, double *result, int acc);
int tlab_zslab_burgers_z(tlab_zslab_plan_t plan, int phase, int nx, int ny, double nu, const double *s, const double *vel,
                         double *head, double *tail, const double *tail_left, const double *head_right, double *result, int acc);
/* nf (1..4) transported fields per launch; head, tail, tail_left, head_right: [nf][2][nx*ny] */
int tlab_zslab_burgers_z_n(tlab_zslab_plan_t plan, int phase, int nx, int ny, int nf, const double *nu, const double *const *s,
                           const double *vel, double *head, double *tail, const double *tail_left, const double *head_right,
                           double *const *result, int acc);
/* phase 2 of d/dz p with the final update of w as its epilogue (as tlab_opr_gradient_final; phase 1 = tlab_zslab_partial_z(plan, 1, ...)) */
int tlab_zslab_gradient_final_z(tlab_zslab_plan_t plan, int nx, int ny, const double *p, const double *tail_left, const double *head_right,
                                double *q, double *h, double dte, double kco, int scale);

/* ---- RHS assembly and Runge-Kutta substep ("next" row n1 of SURVEY.md 8f) --------------------------------- */
/* Module state the reference spreads over TLab_Memory / NavierStokes / OPR_Burgers / BOUNDARY_BCS: plans, sizes,
 * visc = 1/Reynolds, schmidt(1:nscal) (physics/navierstokes.f90), wall boundary conditions (no-slip, Dirichlet scalars). */
typedef struct tlab_dns *tlab_dns_t;
int tlab_dns_create(tlab_dns_t *out, tlab_fdm_plan_t gx, tlab_fdm_plan_t gy, tlab_fdm_plan_t gz,
                    tlab_poisson_plan_t poisson, int nx, int ny, int nz, int nscal, double visc, const double *schmidt);
int tlab_dns_destroy(tlab_dns_t d);
/* on (default): the pointwise sums of the RHS are folded into the operator kernels (same summation order as the reference);
 * off: the reference's literal sequence of temporaries + pointwise loops.  Both give the same result to round-off. */
int tlab_dns_set_fusion(tlab_dns_t d, int on);
/* Scalar bounds limiting, [Control] ScalLimit = yes with MinScalar / MaxScalar (DNS_BOUNDS_LIMIT, tools/dns/dns_local.f90:67-90, called after the update
 * of every substep, time.f90:248-250): after s += dte hs, every active scalar becomes min(max(s, lo), hi) at every point, wall planes included; hs is
 * not touched.  n entries (n <= nscal; scalars beyond n are not limited) of active (!= 0: limited), lo, hi.  active == NULL switches limiting off: the
 * kernels of a run without bounds, the results bit for bit.  TLAB_EINVAL: n > nscal, a NaN bound, lo > hi.  tlab_time_substep_incompressible_explicit
 * applies the bounds (in the epilogue of the kernel that finishes each scalar); tlab_rhs_global_incompressible_1 does not update s and does not. */
int tlab_dns_set_scalar_bounds(tlab_dns_t d, int n, const int *active, const double *lo, const double *hi);
/* Buffer zones, [BufferZone] Type = relaxation (tools/dns/boundary_buffer.f90): the sponge layer h = h - tau(jloc) (a - ref) on the size planes next
 * to Jmin (offset 0) or Jmax (offset ny - size) (RELAX_BLOCK, :463-490).  The flow blocks act on (q, hq) inside the RHS, between the last Burgers sum
 * and the pressure forcing, so that the term is projected (rhs_global_incompressible_1.f90:170-172); the scalar blocks act on (s, hs) in the substep,
 * after the RHS with its wall BCs and before the update (time.f90:628-630).  Jmin goes before Jmax.
 *   end: TLAB_BUFFER_JMIN / _JMAX (_IMIN / _IMAX: TLAB_EUNSUPPORTED, x is periodic here); group: TLAB_BUFFER_FLOW (3 fields) / _SCAL (nscal fields);
 *   tau: HOST, (size, nfields) column-major, see the tau routine below; ref: HOST, (nx, size, nz, nfields), copied into device memory the driver owns.
 *   size = 0 or tau = NULL switches that block off; with every block off the driver launches the kernels of a run without zones, the results bit for bit.
 *   TLAB_EINVAL: nfields other than 3 / nscal, size = 1 (the reference allocates tau and never sets it there, :360), size > ny, NaN in tau.
 * The single-domain driver applies them on both of its routes: the flow blocks in one zone launch between the fused Burgers launches; Dirichlet
 * scalars in the same launch, their wall planes inside a zone redone afterwards (h = 0 - tau (s - ref), update, bounds: zone bytes only); scalars with
 * Neumann walls or a surface model in the reference's literal order (wall planes of hs, zone launch, update: one more pass over them).
 * The type routine mirrors the ini key: TLAB_BUFFER_NONE (switches every block off), _RELAX; _FILTER and _BOTH: TLAB_EUNSUPPORTED.
 * The z-slab and the x/z pencil drivers carry them too (their own setters below). */
#define TLAB_BUFFER_NONE 0
#define TLAB_BUFFER_RELAX 1
#define TLAB_BUFFER_FILTER 2
#define TLAB_BUFFER_BOTH 3
#define TLAB_BUFFER_IMIN 1
#define TLAB_BUFFER_IMAX 2
#define TLAB_BUFFER_JMIN 3
#define TLAB_BUFFER_JMAX 4
#define TLAB_BUFFER_FLOW 0
#define TLAB_BUFFER_SCAL 1
int tlab_dns_set_buffer_type(tlab_dns_t d, int type);
int tlab_dns_set_buffer_zone(tlab_dns_t d, int end, int group, int size, int nfields, const double *tau, const double *ref);
/* INI_BLOCK's strength of one field (:359-371), host arithmetic only: with L = nodes[offset + size - 1] - nodes[offset],
 * form 1 (Jmin): tau[jloc] = strength ((nodes[offset + size - 1] - nodes[j]) / L) ** sigma; form 2 (Jmax): strength ((nodes[j] - nodes[offset]) / L) ** sigma,
 * j = offset + jloc, in the reference's operation order.  nodes: n HOST values; tau_out: size HOST values.  size < 2: TLAB_EINVAL. */
int tlab_buffer_tau(int n, const double *nodes, int offset, int size, double strength, double sigma, int form, double *tau_out);
/* BOUNDARY_BUFFER_RELAX_FLOW (:440-459) and BOUNDARY_BUFFER_RELAX_SCAL (:399-418), incompressible branch, on their own: the driver's blocks applied
 * to HOST arrays of DEVICE pointers (q[3], hq[3]; s[nscal], hs[nscal]).  Planes outside the zones are neither read nor written. */
int tlab_dns_buffer_relax_flow(tlab_dns_t d, double *const *q, double *const *hq);
int tlab_dns_buffer_relax_scal(tlab_dns_t d, double *const *s, double *const *hs);
/* Body forces, [Rotation] and [BodyForce]: TLab_Sources_Flow (src/physics/tlab_sources.f90:36-92), which the reference's substep calls on (q, s, hq)
 * before the RHS (tools/dns/time.f90:610-612).  One kernel launch applies both: Rotation_Coriolis (rotation.f90:103-143) first, then
 * hq_i = hq_i + g_i b for every g_i != 0 with b of Gravity_Buoyancy (gravity.f90:232-342), unfused multiplies and adds in the reference's order.
 *   Coriolis: type TLAB_COR_EXPLICIT (vector = f already divided by Rossby: hq1 = (hq1 + f3 v) - f2 w, and cyclic) or TLAB_COR_NORMALIZED
 *     (hq1 += f2 (geo_w - w), hq3 += f2 (u - geo_u), geo_u = cos(p1) p2, geo_w = -sin(p1) p2 formed on the host; vector (0, f2, 0) only: f1 or f3 != 0
 *     is TLAB_EINVAL, the reference stops there).  parameters: 2 values, read for _NORMALIZED only.
 *   Buoyancy: vector = g already divided by Froude; nscalars = buoyancy%scalar(1); parameters: nparameters HOST values (those beyond read as zero);
 *     inb_scal_array: for TLAB_BOD_LINEAR the independent term is parameters[inb_scal_array] (gravity.f90:253); bbackground: ny HOST values, copied,
 *     or NULL for zeros.  TLAB_BOD_HOMOGENEOUS b = p1; _LINEAR b = ((c1 s1 + c2 s2) + c3 s3) - (ref(j) - c0) with 1..3 scalars, the general branch
 *     (:279-291) otherwise (at most 6 scalars with a factor above small_wp: more is TLAB_EUNSUPPORTED); _BILINEAR b = ((c0 s1 + c1 s2) + (c2 s1) s2) - ref(j); _QUADRATIC
 *     b = (c0 s1)(s1 - c1) - ref(j), c0 = -p1 / (p2/2)^2.
 *   TLAB_EUNSUPPORTED, nothing stored: _EXPLICIT (Thermo_Anelastic_BUOYANCY), _NORMALIZEDMEAN and _SUBTRACTMEAN (they need the plane means FI_DIAGNOSTIC
 *     refreshes every substep), nscalars > nscal on a driver without a mixture (no diagnostic array is held then), nscalars > nscal + 1 with one
 *     (tlab_dns_set_mixture below: the liquid is entry nscal of s, and a linear buoyancy may carry a coefficient for it).
 *   TLAB_EINVAL: an unknown type, NaN or infinite values, a null handle, a type that reads scalars on a driver without them.  The arguments are
 *     checked before the handle.  Type 0 switches the term off; with both off, or all vectors zero, the driver launches the kernels of a run without
 *     forces, the results bit for bit.
 * tlab_time_substep_incompressible_explicit applies them once: on the fused routes where the flow buffer-zone launch goes (every tendency holds a
 * partial sum, none is finished; q and s are those from before the update), on the literal routes after the Burgers sums; always before the pressure
 * forcing and the wall planes of hq2 that become the Neumann data of the Poisson solver, so the force is projected.  Against the reference the terms
 * are summed in another order: rounding only.  tlab_rhs_global_incompressible_1 does not apply them (the reference's RHS does not either).
 * Not built: subsidence, SpecialForcing, Gravity_Buoyancy_Source, the statistics' buoyancy; of TLab_Sources_Scal the gray-liquid infrared term is
 * built (tlab_dns_set_infrared below), gray and band infrared, sedimentation and chemistry are not. */
#define TLAB_COR_NONE 0
#define TLAB_COR_EXPLICIT 4
#define TLAB_COR_NORMALIZED 12
#define TLAB_BOD_NONE 0
#define TLAB_BOD_EXPLICIT 4
#define TLAB_BOD_HOMOGENEOUS 5
#define TLAB_BOD_LINEAR 6
#define TLAB_BOD_BILINEAR 7
#define TLAB_BOD_QUADRATIC 8
#define TLAB_BOD_NORMALIZEDMEAN 9
#define TLAB_BOD_SUBTRACTMEAN 10
int tlab_dns_set_coriolis(tlab_dns_t d, int type, const double *vector, const double *parameters);
int tlab_dns_set_buoyancy(tlab_dns_t d, int type, const double *vector, int nscalars, const double *parameters, int nparameters, int inb_scal_array,
                          const double *bbackground);
/* TLab_Sources_Flow on its own: hq += the terms above and nothing else.  HOST arrays of DEVICE pointers q[3], s[nscal], hq[3]; a component no force
 * touches is neither read nor written, a velocity or scalar no active term needs is not read.  At most 2^31 - 1 points. */
int tlab_dns_sources_flow(tlab_dns_t d, double *const *q, double *const *s, double *const *hq);
/* FI_PRESSURE_BOUSSINESQ(q, s, p, tmp1, tmp2, tmp, decomposition)   physics/fi_pressure_boussinesq.f90:8-280 -- the pressure of a velocity field,
 * what DNS_STATISTICS_TEMPORAL (dns_statistics.f90:93), planes.f90, visuals.f90, averages.f90, pdfs.f90 and spectra.f90 call first.  q[3], s[nscal
 * (+ 1 with a mixture)], tmp[ntmp]: HOST arrays of DEVICE pointers; p, tmp1, tmp2 and every tmp[i] hold isize_txc_field = (nx+2)*ny*nz doubles, as
 * for tlab_opr_poisson.  ntmp >= 3; >= 7 for DCMP_ADVECTION and DCMP_DIFFUSION.  The codes are the reference's (include/dns_const.h:30-36);
 * DCMP_RESOLVED (1) is not a case of the routine: it and any other value are TLAB_EINVAL, as are a null pointer and too few work arrays.
 * In the reference's order: the three sums tmp[0..2] are zeroed; TLab_Sources_Flow is added (DCMP_TOTAL only: every other decomposition zeroes the
 * sums again, :74-86); the nine OPR_Burgers terms are added (x, y, z of each component, bcs = 0); div of the sums by OPR_P1; the wall planes of
 * the second sum are the Neumann data; OPR_Poisson(BCS_NN); OPR_FILTER(p) where a [PressureFilter] is set.  No buffer zone acts (the routine has
 * none), remove_divergence plays no role (no q / dte enters), no scalar equation is launched.
 * The call is a ROUTE through the stages of the substep (csrc/rhs.cpp), with tmp[0..2] in the place of the tendencies and p in that of the forcing:
 * the five- and three-launch Burgers forms, the per-equation sums on the fast kernels and the fused divergence launches serve wherever they serve
 * the substep.  Against the reference, which adds the sources first and then X, Y, Z, those routes add the body forces in the mid-sequence slot and
 * the directions in launch order: rounding only.
 *   DCMP_DIFFUSION  the same launches with an all-zero advecting velocity (tmp[6], the reference's tmp9 = 0).  The reference AS COMPILED does not
 *                   compute this: its OPR_Burgers ignores the velocity argument under OPR_B_SELF and takes the transposed velocity of the call
 *                   before under OPR_B_U_IN, so its x and y terms still advect; the device computes what the call states.
 *   DCMP_ADVECTION  DCMP_ADVDIFF minus DCMP_DIFFUSION (:145-148): two passes of the Burgers launches, the sums of the second in tmp[3..5].
 *   DCMP_CORIOLIS, DCMP_BUOYANCY  one launch of k_body_force on zeroed sums with the other term switched off.  The reference's DCMP_BUOYANCY
 *                   subtracts bbackground for the y component only (:171-177) where TLab_Sources_Flow subtracts it for all three
 *                   (tlab_sources.f90:68); the device holds one profile: a horizontal gravity component together with a non-zero bbackground is
 *                   TLAB_EUNSUPPORTED under this decomposition.
 * Anelastic runs (the sums weighted by rbackground before their derivative; the wall planes scaled once, by rbackground at the wall) and the
 * staggered pressure grid (the sums and the planes interpolated onto the pressure nodes, p back by OPR_P0_INT_PV along z, then x, :272-275) take
 * the literal stages.  Work arrays a route needs beyond the caller's are the library's, allocated on first use and kept with the driver.
 * q, s, hq, hs and the driver's state are unchanged: the one-shot flag of tlab_dns_begin_step is neither read nor consumed.  A recorded substep
 * runs first; like tlab_dns_sources_flow the call returns with its launches enqueued on the library's stream. */
#define TLAB_DCMP_TOTAL 0
#define TLAB_DCMP_ADVECTION 2
#define TLAB_DCMP_ADVDIFF 3
#define TLAB_DCMP_DIFFUSION 4
#define TLAB_DCMP_CORIOLIS 5
#define TLAB_DCMP_BUOYANCY 6
int tlab_dns_pressure(tlab_dns_t d, int decomposition, double *const *q, double *const *s, double *p, double *tmp1, double *tmp2, double *const *tmp,
                      int ntmp);
/* Cloud-top physics of the single-domain driver: [Thermodynamics] Type = Linear, Mixture = AirWaterLinear, and [Infrared] Type = Bulk1dLocal
 * (which the reference maps to grayliquid) -- examples/Case16-21, 54, 55.
 *   Mixture: TLAB_MIXT_NONE or TLAB_MIXT_AIRWATERLINEAR (the reference's MIXT_TYPE_AIRWATER_LINEAR) with thermo_param(1:nparam), HOST values,
 *     nparam >= nscal + 1.  With a mixture the driver has inb_scal_array = nscal + 1: EVERY entry point that takes s then reads nscal + 1 device
 *     pointers, the last the liquid -- the host's contiguous s(isize_field, inb_scal_array); hs stays at nscal.  Other mixtures: TLAB_EUNSUPPORTED;
 *     a driver without scalars, NaN / infinite parameters, nparam < nscal + 1: TLAB_EINVAL.  TLAB_MIXT_NONE also switches the infrared term off, and
 *     is TLAB_EINVAL while a buoyancy that reads the liquid is set.
 *   tlab_dns_diagnostic = FI_DIAGNOSTIC (physics/fi_diagnostic.f90:44-47): the liquid from the prognostic scalars, THERMO_AIRWATER_LINEAR
 *     (thermodynamics/thermo_airwater.f90:483-516) in one pointwise launch (k_airwater_linear): xi = 1 + p1 s1 [+ p2 s2]; l = max(xi, 0) when
 *     |p(nscal+1)| < small_wp, else l = d log(exp(xi (1/d)) + 1), d = p(nscal+1); the reference's operation order, unfused, and nothing beyond its
 *     expression: where exp overflows (xi / d > 709.78) l is infinite, as in the reference.  No mixture: nothing is launched.
 *     tlab_time_substep_incompressible_explicit refreshes the liquid once at its end, after s += dte hs (time.f90:248); the caller makes it valid before
 *     the first substep.  tlab_rhs_global_incompressible_1 does not refresh it (the reference's RHS does not either).  The reference computes the liquid
 *     from the unclipped scalars and clips afterwards (time.f90:248-250), the fused epilogues here clip first: a substep with a mixture AND active scalar
 *     bounds returns TLAB_EUNSUPPORTED.  tlab_dns_place_arrays / _place_blocks place nscal scalar arrays and refuse a driver with a mixture.
 *   Infrared: type TLAB_IR_NONE (switches the term off) or TLAB_IR_GRAY_LIQUID, with the values Radiation_Initialize leaves: scalar = the 1-based
 *     equation the term acts on (infraredProps%active), kappa = kappa(1,1), flux_top = auxiliar(1), flux_bottom = auxiliar(2).  The absorbing field is
 *     always the liquid (infraredProps%scalar(1) = inb_scal_array).  TLAB_EUNSUPPORTED, nothing stored: types 2, 3 (gray, band: they need a temperature
 *     the reference derives for anelastic runs only), an anelastic driver, a y plan whose first-order integral is not the pentadiagonal system of
 *     CompactJacobian6.  TLAB_EINVAL, nothing stored: no mixture (the reference stops there), scalar outside 1..nscal, NaN / infinite values.
 *   tlab_dns_sources_scal = TLab_Sources_Scal (physics/tlab_sources.f90:152-168) on its own: hs[scalar-1] += source and nothing else; s is only read;
 *     txc[0] is scratch, and txc[1] as well when flux_bottom != 0 (no other txc array is touched).  Radiation_Infrared_Y, TYPE_IR_GRAY_LIQUID
 *     (physics/radiation.f90:265-283) with IR_RTE1_OnlyLiquid (:401-444), per (i, k) column in the reference's operation order: a = kappa l;
 *     tau = FDM_Int1_Solve(fdm_Int0(BCS_MAX)) of a with tau(ny) = 0; f = exp(tau); source = a f flux_top, or a (f flux_top + f(1) / f flux_bottom) when
 *     |flux_bottom| > 0.  One launch (k_infrared_y, csrc/radiation.hip), one thread per column: a 2-D run (nz = 1) has few columns and runs slowly but
 *     correctly.
 *   tlab_time_substep_incompressible_explicit applies the source once, from the s of before the update, where the body forces go: hs[scalar-1] holds a
 *     valid partial sum and the launch that finishes that scalar has not run (fused routes), after the Burgers sums (literal routes).  Against the
 *     reference, which adds it before the RHS (tools/dns/time.f90:611), the terms are summed in another order: rounding only.  With the term off there
 *     is no launch and the results are those of a run without it, bit for bit.  tlab_rhs_global_incompressible_1 applies no source.
 * Single-domain driver only: the slab and pencil drivers have no such setters, and no record of the deferred tail carries the source (a host with
 * [Infrared] keeps tlab_deferred_enable off). */
#define TLAB_MIXT_NONE 0
#define TLAB_MIXT_AIRWATERLINEAR 12
#define TLAB_IR_NONE 0
#define TLAB_IR_GRAY_LIQUID 1
int tlab_dns_set_mixture(tlab_dns_t d, int mixture, const double *thermo_param, int nparam);
int tlab_dns_diagnostic(tlab_dns_t d, double *const *s);
int tlab_dns_set_infrared(tlab_dns_t d, int type, int scalar, double kappa, double flux_top, double flux_bottom);
int tlab_dns_sources_scal(tlab_dns_t d, double *const *s, double *const *hs, double *const *txc);
long long tlab_dns_info(tlab_dns_t d, int what);      /* 0 nx, 1 ny, 2 nz, 3 nscal, 4 points of a field, 5 inb_scal_array (arrays in s); -1: null handle or unknown code */
/* Lagrangian particles of the single-domain driver: [Particles] Type = Tracer | Inertia (examples/Case51-53; Case54, 55 use BilinearCloudFour, which is refused), as the serial branch of the reference
 * does them.  The host's particle arrays live in DEVICE memory: l_q and l_hq are HOST arrays of inb_part DEVICE pointers, the columns
 * l_q(isize_part, is) as q and s are passed (inb_part = 3 for tracers: position; 6 for inertial particles: position, velocity); nodes is
 * l_g%nodes (32-bit, 1-based: the y node below the particle), tags is l_g%tags (64-bit).  np is l_g%np, at most 2^31 - 1.  Every entry runs on the
 * library's stream, after a recorded deferred substep.
 *   tlab_dns_set_particles: type TLAB_PART_* (part%type), bcs TLAB_PART_BCS_* (part_bcs; bcs < 0: the reference's default for the type, none for
 *     tracers, specular for inertial particles, particle_procs.f90:65-67), stokes and settling of [Parameters].  TLAB_PART_NONE takes the particles
 *     off the driver again and reads nothing else.  The nodes of the driver's y plan go into a device table here.  TLAB_EUNSUPPORTED, nothing stored:
 *     types 4, 5, 6 (the bilinear cloud droplets need Laplacians, FI_GRADIENT and the radiation at the particle) and an anelastic driver.
 *     TLAB_EINVAL, nothing stored: unknown codes, inertial particles with stokes <= 0, NaN or infinite values, a null handle, plans without nodes.
 *     The arguments are checked before the handle.  A driver on which it was never called launches exactly the kernels of before.
 *   tlab_dns_particle_locate = LOCATE_Y (utils/locate_y.f90) on its own: nodes(p) from y_part(p) (DEVICE arrays) by the reference's own bisection,
 *     which decides the answer for a particle on a node or outside the grid; always 1 <= nodes(p) <= ny - 1.  The host calls it once after
 *     Particle_Initialize_Fields or a restart.
 *   tlab_dns_substep_particle = TIME_SUBSTEP_PARTICLE (tools/dns/time.f90:906-1070, serial branch) and the scaling of l_hq (:300-304) in ONE launch
 *     (k_particle_substep, csrc/particles.hip), one thread per particle:
 *       1. u, v, w at the particle (FIELD_TO_PARTICLE, particle_interpolate.f90:186-332): trilinear from the eight corners of the cell
 *          (floor(x nx / scale_x), nodes(p), floor(z nz / scale_z)), the reference's expression left to right.  The last cell of a periodic direction
 *          takes index 1 as its upper corner (no halo arrays, no particle sorting: same values); a particle exactly at x = scale takes f(nx) with
 *          fraction 0, as in the reference.  nz = 1: the bilinear branch, z is neither interpolated nor wrapped.
 *       2. RHS_PART_1 (rhs_part_1.f90): tracers l_hq(1:3) += (u, v, w); inertial particles l_hq(1:3) += l_q(4:6), l_hq(4:6) += (1/stokes)
 *          ((u, v, w) - l_q(4:6)), l_hq(5) -= settling/stokes (the reference's l_txc is three registers).
 *       3. l_q(is) += dte l_hq(is), is = 1..inb_part.
 *       4. periodic wraps in x and z: > x(1) + scale subtracts scale, < x(1) adds it, one wrap at most.
 *       5. the walls in y: none; stick (y is set onto the wall); specular (y is reflected and l_q(5) changes sign -- a tracer has no fifth
 *          column, so specular only reflects its position).
 *       6. nodes(p) = LOCATE_Y of the new y.
 *       7. l_hq(is) *= kco when scale_tendencies != 0 (every substep but the last).
 *     Unfused multiplies and adds in the reference's order: the numpy restatement (tests/particles_oracle.py) gives the same bits.  It reads q (HOST
 *     array of the 3 DEVICE velocity pointers) and writes no field: call it BEFORE the flow substep of the same stage, as time.f90:231-233 does.
 *     Positions the host hands over are trusted to lie in the box, but no position or node number can take a load outside the fields (the cell
 *     indices are clamped).  TLAB_EINVAL: a driver without particles, np < 0 or > 2^31 - 1, null pointers with np > 0, NaN dte or kco.  np = 0
 *     succeeds without a launch.
 *   tlab_dns_particle_sort: permutes l_q, l_hq, nodes and tags together so that particles are ordered by the cell that holds them, key
 *     (k0 ny + j0) nx + i0 of the current positions and nodes (the whole cell number: the 64 particles of a wave then lie along an x row, whose
 *     corners are contiguous, and a 32-bit key costs the radix sort no more passes coarse than fine); equal keys keep their order.  The reference
 *     itself permutes its particles every substep (particle_interpolate.f90:337-411) and carries tags for identity: order is not part of the state,
 *     and a substep after the sort gives every particle (by tag) the bits it would have got unsorted.  rocPRIM device radix sort of (key, index)
 *     pairs, then one gather per array through the scratch.  scratch: DEVICE memory on a 256-byte boundary.  The size query is a call with
 *     scratch = NULL: *scratch_needed receives the bytes for np particles and nothing is sorted (scratch_needed may be NULL otherwise).  Scratch that
 *     is too small or misaligned: TLAB_EINVAL, the arrays untouched.  The substep never sorts on its own: the host calls this every so many steps.
 * Not built: the slab and pencil drivers (migration between ranks), particle and trajectory files (io_particle.f90, ParticleTrajectories_Write:
 * IO stays on the host), the particle pdfs and residence times (they read the cloud droplets' columns), an order-independent deposit. */
#define TLAB_PART_NONE 0      /* PART_TYPE_*: particle_vars.f90:8-14 */
#define TLAB_PART_TRACER 1
#define TLAB_PART_INERTIA 2
#define TLAB_PART_BCS_NONE 0  /* PART_BCS_*: particle_vars.f90:28-30 */
#define TLAB_PART_BCS_STICK 1
#define TLAB_PART_BCS_SPECULAR 2
int tlab_dns_set_particles(tlab_dns_t d, int type, int bcs, double stokes, double settling);
int tlab_dns_particle_locate(tlab_dns_t d, long long np, const double *y_part, int *nodes);
int tlab_dns_substep_particle(tlab_dns_t d, double dte, double kco, int scale_tendencies, long long np, double *const *q, double *const *l_q,
                              double *const *l_hq, int *nodes);
int tlab_dns_particle_sort(tlab_dns_t d, long long np, double *const *l_q, double *const *l_hq, int *nodes, long long *tags, void *scratch,
                           long long scratch_bytes, long long *scratch_needed);
/* Transfers between the particles and the grid (csrc/particles.hip), for a driver with particles (tlab_dns_set_particles); l_q, nodes, tags and np as
 * above (the positions are the first three columns of l_q), one thread per particle, the weights and corners of step 1 of the substep: the seam
 * cell's upper corner is index 1, a particle at x = scale lies in cell nx with fraction 0, and no position (NaN included) or node number can take a
 * load or a store outside the arrays.  Every entry runs on the library's stream, after a recorded deferred substep, and writes no state of the
 * driver.  TLAB_EINVAL, nothing written: a driver without particles, np < 0 or > 2^31 - 1, null pointers with np > 0, and what each entry lists.
 * np = 0 succeeds without a launch.
 *   tlab_dns_field_to_particle = FIELD_TO_PARTICLE (particle_interpolate.f90:186-332) of nvar >= 1 fields: fields and out are HOST arrays of nvar
 *     DEVICE pointers (fields of nx ny nz, particle arrays of np).  Additive as in the reference, out[v](p) = out[v](p) + A (+ B) in the operation
 *     order of the substep's interpolation (bit for bit tests/particles_oracle.py's interpolate), the weights formed once per particle
 *     (k_particle_sample, 8 fields per launch).  TLAB_EINVAL also: nvar < 1.
 *   tlab_dns_set_trajectories: the ntraj tags to be tracked (l_traj_tags, HOST array; distinct, >= 1), kept on the device as a table of (tag, row j)
 *     sorted by tag.  ntraj = 0 removes the table; taking the particles off the driver removes it too.  The reference's default list (TrajFileName =
 *     void: 1 + (j - 1) (isize_part_total / isize_traj), particle_trajectories.f90:114-122) is the caller's to build.  TLAB_EINVAL, the old table
 *     kept: ntraj < 0, a tag below 1 or listed twice.
 *   tlab_dns_trajectories_accumulate = ParticleTrajectories_Accumulate (particle_trajectories.f90:156-230) for column `counter` (1-based, <= nsave)
 *     of l_traj(ntraj + 1, nsave, inb_part + nvar), fp32, column-major, DEVICE memory: row 1 of every variable gets SNGL(rtime); row 1 + j gets
 *     SNGL(l_q(i, iv)) of the particle i that carries tag j for the inb_part prognostic columns, and behind them the value at that particle of each
 *     of the nvar >= 0 fields (HOST array of DEVICE pointers; TRAJ_TYPE_EULERIAN with q and s; for TRAJ_TYPE_VORTICITY the caller makes the
 *     curl with the operators), interpolated onto a zero target.  Each particle looks its tag up by bisection in the table, and only those that
 *     find it interpolate and store (k_particle_trajectories): the tags may be in any order, e.g. after tlab_dns_particle_sort.  The fp32 values are
 *     the round-to-nearest conversions of the oracle's doubles.  A tracked tag that no particle carries leaves its row untouched, and so is every
 *     other column of l_traj.  TLAB_EINVAL also: no table, nvar < 0, counter outside 1 .. nsave, NaN rtime.
 *   tlab_dns_particle_to_field = PARTICLE_TO_FIELD (particle_to_field.f90:12-154): field (DEVICE, nx ny nz) is zero-filled (also for np = 0) and
 *     every particle adds property(p) cube length, the products of :131-147 in that order, to the eight corners of its cell (nz = 1: four).
 *     property: DEVICE array of np, or NULL for 1.0 (the particle number density).  periodic != 0: what falls on the upper corners of the seam cells
 *     is added to index 1 of that direction, which is what the decomposed reference does (it sends column imax + 1 and plane kmax + 1 to the
 *     neighbour) and what conserves sum(property); periodic = 0: it is dropped, as the serial reference does when it copies (1:imax, 1:kmax) out
 *     of its extended array.  The sums are no-return fp64 atomic adds at agent scope (k_particle_deposit; field must be ordinary device memory, as
 *     all arrays of this library are), after the particles of adjacent lanes in the same cell have been summed in the wave.  THE ORDER OF THE ADDS
 *     IS THE ORDER OF ARRIVAL: a node that receives more than one contribution differs from the reference's particle-ordered loop, and from
 *     another call on the same input, in rounding only, |difference| <= 2 (cnt - 1) 2^-53 sum |contribution| for cnt contributions; a node that
 *     receives one has the reference's bits.  TLAB_EINVAL also: field NULL. */
int tlab_dns_field_to_particle(tlab_dns_t d, int nvar, const double *const *fields, long long np, double *const *l_q, const int *nodes,
                               double *const *out);
int tlab_dns_set_trajectories(tlab_dns_t d, long long ntraj, const long long *tags);
int tlab_dns_trajectories_accumulate(tlab_dns_t d, double rtime, long long counter, long long nsave, long long np, double *const *l_q,
                                     const int *nodes, const long long *tags, int nvar, const double *const *fields, float *l_traj);
int tlab_dns_particle_to_field(tlab_dns_t d, long long np, double *const *l_q, const int *nodes, const double *property, int periodic,
                               double *field);
/* Start of a Runge-Kutta step: TIME_RUNGEKUTTA sets hq = 0, hs = 0 there (tools/dns/time.f90:212-216).  Instead of filling the arrays,
 * tell the driver: the next tlab_rhs_global_incompressible_1 / tlab_time_substep_incompressible_explicit treats them as zero (its first
 * operator launch overwrites instead of accumulating), whatever they contain. */
int tlab_dns_begin_step(tlab_dns_t d);

/* ---- The tail of the substep for a host whose time loop is NOT patched (csrc/deferred.cpp) ---------------------------------------------------
 * tools/dns/time.f90 calls RHS_GLOBAL_INCOMPRESSIBLE_1() (:612), then DAXPY(n, dte, hq(1,is), 1, q(1,is), 1) per field (:649-660) and, in every
 * substep but the last, DSCAL(n, kco, hq(1,is), 1) per field (:279-293); `hq = 0 ; hs = 0` opens a step (:212-216).  Executed one by one the BLAS
 * calls are 2 (3 + ns) passes over the fields.  With tlab_deferred_enable(1) the entry points below only RECORD: when the recorded sequence is
 * exactly that of time.f90 (the tendencies and states the RHS was given, dte as the factor, one kco for all) the library runs ONE
 * tlab_time_substep_incompressible_explicit(dte, kco, scale) -- the call of the patched host, bit for bit -- and the
 * zero fills become tlab_dns_begin_step.  Anything else is executed literally in the order it came.  A recorded sequence runs before any other
 * launch of the library (every entry point that enqueues work, tlab_sync, the copies, tlab_free and the *_destroy functions flush first) and with the
 * settings of the moment it was recorded (every setter whose state a substep reads flushes first as well).  NOT covered: host statements that
 * read a device array directly without a call into the library -- call tlab_deferred_flush() (or tlab_sync()) before them.  A recorded substep that
 * FAILS when another entry point makes it run has no caller to report to: its code is returned by the next tlab_sync / tlab_deferred_flush (the text
 * stays in tlab_last_error()).  Off by default:
 * the four operations then execute immediately (tlab_rhs_global_incompressible_1, tlab_pw_rk_update, tlab_pw_scale, tlab_pw_fill). */
int tlab_deferred_enable(int on);
int tlab_deferred_rhs(tlab_dns_t d, double dte, double *const *q, double *const *s, double *const *hq, double *const *hs, double *const *txc);
int tlab_deferred_axpy(long long n, double a, const double *x, double *y);      /* DAXPY with unit strides: y += a x */
int tlab_deferred_scal(long long n, double a, double *x);                       /* DSCAL with unit stride:  x *= a   */
int tlab_deferred_zero(double *a, long long n);                                 /* a(1:n) = 0                        */
int tlab_deferred_flush(void);
/* DNS_BOUNDS_LIMIT of an unchanged host (time.f90:248-250, dns_local.f90:67-90, through tlab_amd/fortran/dns_local_device.sed): x = min(max(x, lo), hi).
 * Recorded like the BLAS calls: the sequence RHS, DAXPY x (3 + ns), one clip per limited s, [DSCAL x (3 + ns)] runs as ONE fused substep with those
 * bounds (tlab_deferred_stats counts[0]; tlab_deferred_clip_stats counts[0]).  A clip of another array, before the DAXPY of its field, a second clip of one field, or bounds of a driver that has
 * its own (tlab_*_set_scalar_bounds) make the record run literally, in the order of the calls.  Off: tlab_pw_clip. */
int tlab_deferred_clip(long long n, double lo, double hi, double *x);
/* BOUNDARY_BUFFER_RELAX_SCAL of an unchanged host (time.f90:628-630, through tlab_amd/fortran/boundary_buffer_device.sed), on the arrays of the
 * driver's last deferred RHS.  The sequence RHS, relaxation, DAXPY x (3 + ns), [clips], [DSCAL x (3 + ns)] runs as ONE fused substep with the
 * driver's scalar blocks in it; the RHS applies the flow blocks itself.  A relaxation after a DAXPY, a second one, or one on a driver without scalar
 * zones makes the record run literally, in call order.  A record WITHOUT the relaxation is replayed without the scalar blocks, fused or literal.
 * The relax statistics give counts[2]: fused substeps that carried a recorded relaxation, relaxations executed on their own. */
int tlab_deferred_relax_scal(tlab_dns_t d);
int tlab_deferred_relax_stats(long long *counts);
/* TLab_Sources_Flow of an unchanged host (time.f90:610, through tlab_amd/fortran/tlab_sources_device.sed).  Layer off: tlab_dns_sources_flow.  On: a
 * pending record runs first and the call is kept as a marker.  A tlab_deferred_rhs of the same driver on the same arrays straight after it makes the
 * record sources, RHS, [relaxation], DAXPY x (3 + ns), [clips], [DSCAL x (3 + ns)], which runs as the ONE fused substep with the forces in it.  A
 * record WITHOUT the marker is replayed without forces.  Anything else -- another driver, other arrays, a second marker, something that wants the
 * stream while only the marker is pending -- makes the marker run literally, in call order, after REAL zero fills where zero fills were recorded.
 * The statistics give counts[2]: fused substeps that carried the marker, markers executed on their own. */
int tlab_deferred_sources_flow(tlab_dns_t d, double *const *q, double *const *s, double *const *hq);
int tlab_deferred_sources_stats(long long *counts);
/* counts[6]: fused substeps run, sequences executed literally, begin_steps taken from zero fills, eager axpy, eager scal, eager zero fills */
int tlab_deferred_stats(long long *counts);
/* counts[2]: fused substeps that carried recorded clips (of counts[0] above), clips executed on their own (tlab_pw_clip) */
int tlab_deferred_clip_stats(long long *counts);
/* 1: p points into device memory, 0: host memory, < 0: error.  tlab_deferred_axpy / tlab_deferred_scal use it as a guard, so that a BLAS-1 call of the
 * host on host arrays (the DAXPY / DSCAL of tlab_amd_dns.f90 are global symbols) never reaches a kernel: host + host runs as a host loop at once,
 * device + device as before, mixed pointers are refused (TLAB_EINVAL).  The ranges seen last are cached. */
int tlab_pointer_on_device(const void *p);
/* Which device allocations should play q, s, hq, hs, txc?  The rate of a kernel that streams many arrays at once depends on the SET of allocations
 * it streams (not on any one of them): 4.8 .. 5.9 TB/s for one 13-stream kernel over sets of 1-GiB hipMalloc allocations, 16.0 .. 17.2 ms per substep
 * of the 512^3 box from process to process (profiles/r05/placement_*.txt).  No rule predicts it, so it is searched: given a pool
 * of npool >= 2 (3 + nscal) + 9 candidate arrays, each of at least isize_txc_field doubles, the substep itself (one three-stage Runge-Kutta step per
 * trial, timed by events) is run on the assignment "pool in order", on random_trials random assignments and on one pass of single-role exchanges,
 * and the fastest comes back: assignment[r] = index into pool of role r, roles in the order q[0..2], s[0..nscal-1], hq[0..2], hs[0..nscal-1],
 * txc[0..8].  state: 3 + nscal device arrays the trial fields start from (NULL: zeros).  EVERY array of the pool is overwritten; the caller puts its
 * fields into the chosen arrays afterwards.  report (NULL or 5 doubles): ms per substep of the first assignment, the best, the median, the worst,
 * and the number of trials.  A start-up cost of (random_trials + nroles + 1) x 4 substeps; the results of the run do not depend on it. */
int tlab_dns_place_arrays(tlab_dns_t d, int npool, double *const *pool, const double *const *state, double dtime, int random_trials,
                          unsigned seed, int *assignment, double *report);
/* After the search the first assignment and the winner are timed again back to back (three steps each); the winner is kept only if its median is
 * the lower one, and report[0], report[1] come from those repeats.  The begin_step flag of the driver is what it was on entry; the contents of
 * EVERY pool array (state, tendencies, work arrays) are undefined afterwards. */
/* The same search for a host whose arrays are two-dimensional (Tlab: q(isize_field, 3), s(isize_field, ns), hq, hs, txc(isize_txc_field, 9);
 * base/tlab_memory.f90:201-207, dns_main.f90:103-104): components lie a fixed stride apart, so only whole BLOCKS can be placed.  cand_X[0..ncand-1]
 * are candidate allocations for block X (index 0 = what the host holds now; q / hq: 3 n doubles, s / hs: nscal n, txc: 9 txc_stride); the substep
 * is timed on the host's own combination, on random_trials random ones and on one pass of single-block exchanges, the winner confirmed as above.
 * choice[5]: the candidate index per block in the order q, s, hq, hs, txc; report as tlab_dns_place_arrays.  All candidates are overwritten: call
 * it BEFORE the fields are read, then point the host arrays at the chosen allocations and free the others. */
int tlab_dns_place_blocks(tlab_dns_t d, int ncand, double *const *cand_q, double *const *cand_s, double *const *cand_hq, double *const *cand_hs,
                          double *const *cand_txc, long long txc_stride, double dtime, int random_trials, unsigned seed, int *choice, double *report);
/* Wall boundary conditions in y: BcsFlowJmin%type(1:3), BcsFlowJmax%type(1:3), BcsScalJmin%type(1:nscal), BcsScalJmax%type(1:nscal)
 * (tools/dns/boundary_bcs.f90:24-27, read at :102-190).  Values as in the reference: DNS_BCS_DIRICHLET / DNS_BCS_NEUMANN.
 * Default at creation: all Dirichlet ('noslip'; the reference's 'freeslip' is {NEUMANN, DIRICHLET, NEUMANN} for (u,v,w)).
 * The normal velocity (index 1 here, 0-based) must stay Dirichlet: the pressure solver's Neumann data assume v = 0 at the walls. */
#define TLAB_DNS_BCS_DIRICHLET 3
#define TLAB_DNS_BCS_NEUMANN 4
int tlab_dns_set_bcs(tlab_dns_t d, const int *flow_jmin, const int *flow_jmax, const int *scal_jmin, const int *scal_jmax);
/* [PressureFilter] of dns.ini: p and dp/dy pass OPR_FILTER after the Poisson solve (rhs_global_incompressible_1.f90:286-290; examples/Case92-93:
 * compact filter in y with zero ends).  Filters not owned; NULL = none. */
int tlab_dns_set_pressure_filter(tlab_dns_t d, tlab_filter_t fx, tlab_filter_t fy, tlab_filter_t fz, const int *repeat);
/* [Filter] of dns.ini: FilterDomain(1:3) of DNS_FILTER (operators/opr_filter.f90:45, tools/dns/dns_filter.f90).  Filters not owned; NULL = none in
 * that direction, all NULL switches the filter off; repeat may be NULL (once each).  A filter whose size is not the extent along its direction and
 * a Repeat < 1 are refused (TLAB_EINVAL) and leave the driver as it was.  The types are those of tlab_filter_create: tophat and the 3-D types
 * (Helmholtz, band, erf) have no handle (TLAB_EUNSUPPORTED there). */
int tlab_dns_set_filter(tlab_dns_t d, tlab_filter_t fx, tlab_filter_t fy, tlab_filter_t fz, const int *repeat);
/* DNS_FILTER (tools/dns/dns_filter.f90) of the incompressible / anelastic equations, what dns_main.f90 calls every nitera_filter steps after
 * TIME_RUNGEKUTTA, without its kin statistics: OPR_FILTER(FilterDomain) on u, v, w and the nscal prognostic scalars (tlab_opr_filter_fields), then
 * DNS_BOUNDS_LIMIT on the scalars with active bounds (tlab_dns_set_scalar_bounds), then FI_DIAGNOSTIC where a mixture is set (s then holds
 * nscal + 1 arrays, tlab_dns_diagnostic).  Without a filter the last two still act, as in the reference.  q, s: HOST arrays of device pointers.
 * No tendency and no other state of the driver is touched. */
int tlab_dns_filter(tlab_dns_t d, double *const *q, double *const *s);
/* remove_divergence of dns.ini (tools/dns/dns_read_local.f90): on (default): the pressure forcing is div(hq + q/dte), which removes the residual
 * divergence of q (rhs_global_incompressible_1.f90:177-232); off: div(hq) (:234-250). */
int tlab_dns_set_remove_divergence(tlab_dns_t d, int on);
/* Dynamic surface model of the scalars: BcsScalJmin/Jmax%SfcType (0 = DNS_SFC_STATIC, 1 = DNS_SFC_LINEAR) and %cpl per scalar
 * ([BoundaryConditions] Scalar<i>SfcTypeJmin/Jmax, Scalar<i>CouplingJmin/Jmax; tools/dns/boundary_bcs.f90:29-31, 76-87).  With a linear surface the
 * wall plane of the scalar's tendency is its old value plus cpl times the anomaly of the diffusive surface flux: the tendency planes kept at the
 * start of the RHS (rhs_global_incompressible_1.f90:77-87) and BOUNDARY_BCS_SURFACE_Y (boundary_bcs.f90:478-546: d/dy of the scalar, AVG1V2D of its
 * plane j = 1 -- at both ends, as the reference has it) in the boundary section (:393-396).  Single-domain driver (the plane average is an
 * all-reduce in a decomposed run: the slab / pencil drivers do not take it). */
int tlab_dns_set_surface_bcs(tlab_dns_t d, const int *sfc_jmin, const int *sfc_jmax, const double *cpl_jmin, const double *cpl_jmax);
/* nse_eqns == DNS_EQNS_ANELASTIC: the density weights of the RHS (Thermo_Anelastic_WEIGHT_INPLACE / _SUBTRACT with rbackground / ribackground,
 * tools/dns/rhs_global_incompressible_1.f90:211-214, :326-329; the Neumann data of the pressure times rbackground at the walls, :275-277) and of
 * OPR_Burgers (below).  rbackground, ribackground: HOST pointers, ny values each, ribackground = 1 / rbackground -- the profiles the host's
 * thermodynamics made (Thermo_Anelastic is outside the path); NULL switches back to the incompressible equations.  Anelastic substeps take the
 * literal operator sequence (no fused forms). */
int tlab_dns_set_anelastic(tlab_dns_t d, const double *rbackground, const double *ribackground);

/* BOUNDARY_BCS_NEUMANN_Y(ibc, nx, ny, nz, g, u, bcs_hb, bcs_ht, tmp1)   tools/dns/boundary_bcs.f90:368-473
 * Wall values of u (planes of nx*nz, x fastest) such that du/dy = 0 at the bottom (ibc = 1), top (2) or both (3) walls,
 * from the Neumann-reduced first-derivative system of g.  u is read only (its wall planes are not used); a plane not selected
 * by ibc is left untouched; tmp1 is work space of nx*ny*nz. */
int tlab_boundary_bcs_neumann_y(tlab_fdm_plan_t g, int ibc, int nx, int ny, int nz, const double *u, double *bcs_hb,
                                double *bcs_ht, double *tmp1);

/* ---- per-iteration monitors ("next" row n2 of SURVEY.md 8f) -------------------------------------------------------------
 * TIME_COURANT()   tools/dns/time.f90:365-548 (incompressible branch; constants of TIME_INITIALIZE :138-176):
 *   pmax[0] = max |u|/dx + |v|/dy + |w|/dz over the local box, pmax[1] = schmidtfactor * max(1/dx^2 + 1/dy^2 + 1/dz^2);
 *   dtime (may be NULL) = min(cfla / pmax[0], cfld / pmax[1]) if cfla > 0.  With several ranks the caller MPI_MAX-reduces pmax first
 *   (time.f90:522) -- tlab_dns_set_slab tells a z-slab its first global plane (ims_offset_k).  Synchronises the stream.
 * FI_INVARIANT_P(nx,ny,nz,u,v,w,result,tmp1)   mappings/fi_vectorcalculus.f90:111-141 : result = -div(u,v,w)
 * MINMAX(imax,jmax,kmax,a,amn,amx)             utils/minmax.f90:6 (local part; DNS_BOUNDS_CONTROL dns_local.f90:184-187 uses both) */
int tlab_dns_set_slab(tlab_dns_t d, int koffset);
int tlab_time_courant(tlab_dns_t d, double *const *q, double cfla, double cfld, double *pmax, double *dtime);
int tlab_fi_invariant_p(tlab_dns_t d, const double *u, const double *v, const double *w, double *result, double *tmp1);
int tlab_minmax(tlab_dns_t d, const double *a, int nx, int ny, int nz, double *amn, double *amx);
/* FI_VORTICITY(nx,ny,nz,u,v,w,result,tmp1,tmp2)   mappings/fi_vorticity.f90:28-59 : result = (v,x - u,y)^2 + (u,z - w,x)^2 + (w,y - v,z)^2, the
 *   squared magnitude of the vorticity.  Six OPR_Partial(OPR_P1, bcs = 0) with the driver's plans in the reference's order -- v,x  u,y  u,z  w,x
 *   w,y  v,z -- into txc6[0..5] (a HOST array of six DEVICE pointers, nx*ny*nz doubles each, which hold them on return), then ONE pass
 *   (k_vorticity_magnitude) that reads the six and writes ((a-b)*(a-b) + (c-d)*(c-d)) + (e-f)*(e-f), unfused: the reference's operation order, where
 *   the reference makes three two-operand passes over result through two work arrays.  result aliases none of the six.  No IBM.  Returns with the
 *   launches enqueued on the library's stream.
 * tlab_vorticity_from_gradients: that pass on its own, no driver handle, for arrays of either kind (all device -> the kernel, all host or no
 *   tlab_init -> a host loop with the same operations; a mix: TLAB_EINVAL).  16-byte accesses where all seven arrays are 16-byte aligned, 8-byte
 *   accesses otherwise.  1 <= n <= 2^31 - 1. */
int tlab_fi_vorticity(tlab_dns_t d, const double *u, const double *v, const double *w, double *result, double *const *txc6);
int tlab_vorticity_from_gradients(long long n, const double *vx, const double *uy, const double *uz, const double *wx, const double *wy,
                                  const double *vz, double *result);
/* DNS_BOUNDS_CONTROL with the location of its failure branch (tools/dns/dns_local.f90:157-230, incompressible / anelastic):
 *   dil_min, dil_max = min / max of div(q) (= -FI_INVARIANT_P, logs_data(10:11)); loc_min, loc_max (int[3] each; NULL = not wanted) = the 1-based
 *   (i, j, k) of the first occurrence in column-major order (Fortran minloc / maxloc), k offset by tlab_dns_set_slab.  q[3], txc[9]: HOST arrays
 *   of DEVICE pointers; txc[0], txc[5], txc[6] are destroyed (and txc[2..4], which take rbackground * q, in anelastic runs, :160-162).  Staggered
 *   runs (FI_INVARIANT_P_STAG): TLAB_EUNSUPPORTED.  Synchronises the stream.
 * tlab_device_minmax: the local part of MINMAX (utils/minmax.f90:6) on any DEVICE array of n doubles (no driver). */
int tlab_dns_dilatation_extremes(tlab_dns_t d, double *const *q, double *const *txc, double *dil_min, double *dil_max, int *loc_min, int *loc_max);
int tlab_device_minmax(const double *a, long long n, double *amn, double *amx);
/* tlab_minmax_any: the same for an array of either kind, classified by tlab_pointer_on_device: device memory -> the kernel, host memory (or no
 * tlab_init) -> a host loop.  A host array never reaches a kernel. */
int tlab_minmax_any(const double *a, long long n, double *amn, double *amx);

/* ---- plane statistics: module Averages and the covariance blocks of AVG_FLOW_XZ / AVG_SCAL_XZ ------------------------------------------------
 * Profiles in y of fields a(nx, ny, nz), x fastest.  No driver handle.  The fields are classified like tlab_minmax_any: all in device memory -> two
 * kernels (k_plane_partial, k_plane_final: deterministic, no atomics; the order of summation depends on (nx, ny, nz) and the 16-byte alignment of
 * the fields alone, so a call repeats its bits); all in host memory (or no tlab_init) -> a host loop in the reference's order (k outer, i inner for
 * a given j); a mix: TLAB_EINVAL.  Profiles, in and out, are HOST memory, ny doubles per column.  A recorded substep runs first; the calls return
 * with the profile on the host (they synchronise the stream).  The scratch they need is the library's, grown on demand.
 * TLAB_EINVAL: nx, ny or nz < 1, nf < 1, imom outside 1..4, ld < ny, a null pointer (p and rP may be NULL, but only together).
 * tlab_avg_ik_v: AVG_IK_V (utils/averages.f90:301-327), local part, of nf arrays in ONE pass over them: column f of avg, at avg + f*ldavg, is
 *   sum_{i,k} a[f](i, j, k) / real(nx*nz) -- a division, as in the reference.  a: HOST array of nf pointers.
 * tlab_avg1v2d_v: AVG1V2D_V (:142-167), local part: the plane average of a**imom, imom = 1..4, the power as gfortran expands it:
 *   a, a*a, (a*a)*a, (a*a)*(a*a). */
int tlab_avg_ik_v(int nx, int ny, int nz, int nf, const double *const *a, double *avg, int ldavg);
int tlab_avg1v2d_v(int nx, int ny, int nz, int imom, const double *a, double *avg);
/* The covariances of AVG_FLOW_XZ (statistics/avg_flow_xz.f90:513-553, :597-654, incompressible / anelastic branch) in one pass over u, v, w (and p):
 * with u' = u - fU(j), v' = v - fV(j), w' = w - fW(j), p' = p - rP(j), column c of out (at out + c*ldout) is the plane average of
 *   0 Rxx = u'u'      1 Ryy            2 Rzz            3 Rxy = u'v'      4 Rxz = u'w'      5 Ryz = v'w'
 *   6 rU3 = (u'u')u'  7 rU4 = u' (u'u')u'               8 rV3   9 rV4    10 rW3  11 rW4
 *  12 Txxy = (u'u')v' 13 Tyyy = (v'v')v' 14 Tzzy = (w'w')v' 15 Txyy = (u'v')v' 16 Txzy = (u'v')w' 17 Tyzy = (v'v')w'
 *  and with p != NULL   18 rP2 = p'p'   19 u'p'   20 v'p'   21 w'p'
 * each term formed in the reference's operation order, unfused.  What the reference adds on the host afterwards (Ty1, Txyy += <u'p'>, Tyyy +=
 * 2 <v'p'>, Tyzy += <w'p'>) stays with the caller.  18 columns without p, 22 with. */
int tlab_avg_moments_flow(int nx, int ny, int nz, const double *u, const double *v, const double *w, const double *p, const double *fU,
                          const double *fV, const double *fW, const double *rP, double *out, int ldout);
/* The moments and fluxes of one scalar in AVG_SCAL_XZ (statistics/avg_scal_xz.f90:373-455), with s' = s - fS(j):
 *   0 rS2 = s's'   1 rS3 = s'(s's')   2 rS4 = s' s'(s's')   3 Rsu = s'u'   4 Rsv = s'v'   5 Rsw = s'w'
 *   6 Tssy1 = (s'v')s'   7 Tsuy1 = (s'u')v'   8 Tsvy1 = (s'v')v'   9 Tswy1 = (s'w')v'   and with p != NULL   10 Tsvy3 = p's'
 * 10 columns without p, 11 with.  The PIs* terms need derivative fields and are not computed here. */
int tlab_avg_moments_scal(int nx, int ny, int nz, const double *s, const double *u, const double *v, const double *w, const double *p,
                          const double *fS, const double *fU, const double *fV, const double *fW, const double *rP, double *out, int ldout);
/* The groups of AVG_FLOW_XZ on the nine velocity derivatives (Section 3, statistics/avg_flow_xz.f90:988-1248, and the pressure strain :681-699), in
 * three passes over them instead of about 60 temporaries and reductions.  grad: HOST array of 9 pointers dudx dudy dudz dvdx dvdy dvdz dwdx dwdy
 * dwdz; with d = dudx + dvdy + dwdz, c23 = 2.0/3.0, column c of out (at out + c*ldout) is the plane average of
 *  first pass (no means)
 *   0 vortx = dwdy - dvdz   1 vorty = dudz - dwdx   2 vortz = dvdx - dudy
 *   3 Tau_yy = dvdy*2.0 - dudx - dwdz   4 Tau_xy = dudy + dvdx   5 Tau_yz = dvdz + dwdy                                     (RAW)
 *  second pass (means rU_y rV_y rW_y and columns 0-2)
 *   6-32 U_x2 U_x3 U_x4  V_y.  W_z.  U_y.  U_z.  V_x.  V_z.  W_x.  W_y.: a*a, (a*a)*a, ((a*a)*a)*a of a = the derivative, the y-derivatives
 *        minus rU_y / rV_y / rW_y                                                                                           (:1021-1106)
 *   33 U_ii2 = (d - rV_y)*(d - rV_y)          34-36 vortx2 vorty2 vortz2 = (vort - column 0..2)**2                        (:1110, :993-1010)
 *   37 Phi (RAW) = dudx**2 + dvdy**2 + dwdz**2 + 0.5*((dudy+dvdx)**2 + (dudz+dwdx)**2 + (dvdz+dwdy)**2) - d**2/3.0          (:1136)
 *   38-43 Exx Eyy Ezz Exy Exz Eyz (RAW), the expressions of :1145-1176, each with p = d*c23
 *  third pass (means: columns 3-5, fU fV fW (, rP)); t22 = (raw_yy - Tau_yy)*c23, t12 = raw_xy - Tau_xy, t23 = raw_yz - Tau_yz
 *   44 Txxy_v = t12 u'  45 Tyyy_v = t22 v'  46 Tzzy_v = t23 w'  47 Txyy_v = t22 u' + t12 v'  48 Txzy_v = t23 u' + t12 w'
 *   49 Tyzy_v = t23 v' + t22 w'                                                                                          (:1212-1245)
 *   and with p != NULL   50-52 PIxx PIyy PIzz (RAW) = p' dudx, p' dvdy, p' dwdz   53 PIxy = p'(dudy+dvdx)  54 PIxz = p'(dudz+dwdx)
 *   55 PIyz = p'(dvdz+dwdy)                                                                                        (:681-683, :697-699)
 * 50 columns without p, 56 with.  Constant transport: the vis factors of EQNS_TRANS_POWERLAW / SUTHERLAND are not applied.  RAW = before what
 * the reference applies to the profile on the host, which stays with the caller:
 *   Phi = Phi*visc*2 (:1140)   Tau_yy = Tau_yy*visc*c23, Tau_xy = Tau_xy*visc, Tau_yz = Tau_yz*visc (:1187, :1195, :1203)
 *   Txxy -= Txxy_v*visc*2, Tyyy -= Tyyy_v*visc*2, Tzzy -= Tzzy_v*visc*2, Ty3 -= (each of the three)*visc (:1215-1230)
 *   Txyy -= Txyy_v*visc, Txzy -= Txzy_v*visc, Tyzy -= Tyzy_v*visc (:1236-1248)
 *   Exx = (Exx*visc - Tau_xy*rU_y)*2, Eyy = (Eyy*visc - Tau_yy*rV_y)*2, Ezz = (Ezz*visc - Tau_yz*rW_y)*2, Exy = Exy*visc - Tau_xy*rV_y -
 *   Tau_yy*rU_y, Exz = Exz*visc - Tau_xy*rW_y - Tau_yz*rU_y, Eyz = Eyz*visc - Tau_yy*rW_y - Tau_yz*rV_y (:1263-1268, the finished Tau)
 *   PIxx = PIxx*2, PIyy = PIyy*2, PIzz = PIzz*2 (:687-689)
 * tlab_avg_ugradp: the plane average of u*dpdx + v*dpdy + w*dpdz (:673), one column of ny.
 * tlab_avg_gradients_scal: the same for one scalar (statistics/avg_scal_xz.f90); grads: HOST array of 3 pointers dsdx dsdy dsdz
 *   0 Fy (RAW) = dsdy (:738)   1 Ess (RAW) = dsdx*dsdx + dsdy*dsdy + dsdz*dsdz (:607)
 *   2-10 S_x2 S_y2 S_z2 S_x3 S_y3 S_z3 S_x4 S_y4 S_z4, the chains of :714-730, y minus rS_y
 *   11 Tssy2 (RAW) = (dsdy - Fy) s'   12-14 Tsuy2_d Tsvy2_d Tswy2_d = (dsdy - Fy) u', v', w' (:742-745, Fy = column 0)
 *   and with p != NULL (then fS_y is needed too)   15 PIsu = p' dsdx   16 PIsv = p'(dsdy - fS_y)   17 PIsw = p' dsdz (:451-453)
 *   15 columns without p, 18 with.  The caller's lines: Ess = Ess*diff*2 (:610), Tssy2 = -Tssy2*diff*2 (:748), Tsuy2 -= Tsuy2_d*diff, Tsvy2 -=
 *   Tsvy2_d*diff, Tswy2 -= Tswy2_d*diff (:750-754), Fy = Fy*diff (:756). */
int tlab_avg_gradients_flow(int nx, int ny, int nz, const double *const *grad, const double *u, const double *v, const double *w, const double *p,
                            const double *fU, const double *fV, const double *fW, const double *rP, const double *rU_y, const double *rV_y,
                            const double *rW_y, double *out, int ldout);
int tlab_avg_ugradp(int nx, int ny, int nz, const double *u, const double *v, const double *w, const double *dpdx, const double *dpdy,
                    const double *dpdz, double *out);
int tlab_avg_gradients_scal(int nx, int ny, int nz, const double *const *grads, const double *s, const double *u, const double *v, const double *w,
                            const double *p, const double *fS, const double *fU, const double *fV, const double *fW, const double *rP,
                            const double *rS_y, const double *fS_y, double *out, int ldout);
/* One pass of the above on its own, for a decomposed host that reduces the profiles of a pass over its ranks before the next pass takes them as
 * means (AVG_IK_V's MPI_ALLREDUCE): pass 1-3 = the passes of tlab_avg_gradients_flow, 4-5 = those of tlab_avg_gradients_scal; with_p for passes
 * 3 and 5.  fields, means: HOST arrays of pointers in the order the pass reads them; out: the columns of that pass alone, from column 0.
 *   pass  fields                                   means                                      columns
 *   1     the 9 gradients                          -                                          6  (0-5 above)
 *   2     the 9 gradients                          rU_y rV_y rW_y vortx vorty vortz           38 (6-43)
 *   3     the 9 gradients, u v w (, p)             Tau_yy Tau_xy Tau_yz (raw) fU fV fW (, rP)  6 or 12 (44-55)
 *   4     dsdx dsdy dsdz                           rS_y                                       11 (0-10)
 *   5     dsdy s u v w (, p dsdx dsdz)             Fy (raw) fS fU fV fW (, rP fS_y)            4 or 7 (11-17) */
int tlab_avg_gradients_pass(int pass, int with_p, int nx, int ny, int nz, const double *const *fields, const double *const *means, double *out,
                            int ldout);
/* The same on a driver, with the derivatives of Section 3 (:976-986) in front: q[3], txc[9] HOST arrays of DEVICE pointers.  With p the three
 * derivatives of p go to txc[6..8] first (:670-672) and ugradp is written as column 56 (out holds 57 columns then, 50 without p); then the nine
 * OPR_Partial_{X,Y,Z}(OPR_P1) of u, v, w with the driver's plans, bcs = 0, into txc[0..8] = dudx .. dwdz, which hold them on return; then
 * tlab_avg_gradients_flow on them.  tlab_dns_avg_gradients_scal: dsdx dsdy dsdz of s into txc[0..2], then tlab_avg_gradients_scal. */
int tlab_dns_avg_gradients_flow(tlab_dns_t d, double *const *q, const double *p, double *const *txc, const double *fU, const double *fV,
                                const double *fW, const double *rP, const double *rU_y, const double *rV_y, const double *rW_y, double *out,
                                int ldout);
int tlab_dns_avg_gradients_scal(tlab_dns_t d, const double *s, double *const *q, const double *p, double *const *txc, const double *fS,
                                const double *fU, const double *fV, const double *fW, const double *rP, const double *rS_y, const double *fS_y,
                                double *out, int ldout);

/* ---- plane PDFs: module PDFS (utils/pdfs.f90) and PDF1V_N / PDF2V (statistics/pdf.f90), the block stats_pdfs of DNS_STATISTICS ------------------
 * Histograms (counts, not normalised) of fields u(nx, ny, nz), x fastest, in every plane j and -- when ny > 1 -- in the whole volume, written as
 * plane ny + 1.  No driver handle; the conventions of the plane statistics above: all arrays in device memory -> the kernels of csrc/pdfs.hip, all
 * in host memory (or no tlab_init) -> the reference's loops on the host; a mix: TLAB_EINVAL.  A recorded substep runs first; results are in HOST
 * memory on return; scratch is the library's.  No global atomics, no float atomics: counts are integers (32 bits per workgroup in LDS, 64 bits
 * across workgroups), exact in any order, so a call repeats its bits and they are the reference's while a count stays below 2^53.
 * The bin of a point is up = int(q) + 1, q = (u - umin)/ustep (one subtraction, one division, fp64, unfused), ustep = (umax - umin)/real(nbins)
 * and 1 where that is 0; pdf(nbins+1) = umin + 0.5 ustep, pdf(nbins+2) = umax - 0.5 ustep with the step before that replacement.  int()
 * truncates toward zero: with an external interval a value slightly below umin (q in (-1, 0)) is counted in bin 1 and a value equal to umax is
 * dropped, as in the reference.  Where Fortran's int() is undefined the result is defined: an external interval counts a point iff
 * -1 < q < nbins; a local interval counts every finite q > -1, in bin min(trunc(q) + 1, nbins); NaN and infinite q are dropped.  Fields that hold
 * NaN are OUTSIDE the contract (their min / max are not the reference's).
 * A gate (igate != 0): only points with gate == igate take part (PDF1V2D1G); min and max start from big_wp = 1e20 and -big_wp, and a plane without
 * a gated point goes through the same expressions with those.  gate: int8, the layout of a field; may be NULL when igate == 0.
 * TLAB_EINVAL: nx, ny, nz or nv < 1, nbins < 1 or above the compiled limit 4096, a null field, igate != 0 with a null gate, ibc outside 0..5.
 *
 * tlab_pdf1v_n: the calculation of PDF1V_N (statistics/pdf.f90:14-91; no file is written).  u: HOST array of nv pointers; ibc[nv]: 0 external
 *   interval [umin[v], umax[v]], 1 local interval, 2..5 local interval, then PDF_ANALIZE(ibc - 2, .., plim = 1e-4) of every plane and the histogram
 *   on the analysed interval as an external one.  pdf: (nbins+2, ny+1, nv) doubles, Fortran order; the last plane is zero when ny == 1.  umin,
 *   umax may be NULL when no ibc is 0.  All fields share the passes (min/max; histogram; histogram on the analysed intervals): at most three
 *   device-to-host synchronisations whatever nv and ny.
 * tlab_pdf_minmax_planes, tlab_pdf_histogram_planes: the two passes on their own, for a decomposed host that reduces min / max, then the counts,
 *   over its ranks in between (the MPI_ALLREDUCEs of PDF1V2D).  umin, umax: (ny+1, nv) doubles, the volume's as plane ny+1 (computed also when
 *   ny == 1); ilim[v] == 0: the intervals of field v are external (a point outside is dropped), otherwise local (the last point in the last bin).
 *   pdf as above, bounds included.
 * tlab_pdf_analize: PDF_ANALIZE (utils/pdfs.f90:329-379), host arithmetic on one pdf(nbins+2).
 * tlab_pdf2v: PDF2V (statistics/pdf.f90:123-159) over PDF2V2D, single rank: min / max of u, the min / max of v in every u-bin, the
 *   nbins[0] x nbins[1] histogram with both indices clipped to the last bin.  pdf: (nbins[0]*nbins[1] + 2 + 2*nbins[0], ny+1), bin (up, vp) at
 *   (vp-1)*nbins[0] + up.  nbins[0]*nbins[1] at most 4096, nbins[0] at most 1024.
 * tlab_gate_threshold: gate[i] = a[i] > thr ? 1 : 0 for n points (the gate of dns_statistics.f90:106-110); a and gate of one kind.  On the device
 *   the call returns with the kernel enqueued on the library's stream.
 * tlab_inter_n_xz: the calculation of INTER_N_XZ (statistics/avg_xz.f90:109-153; no file is written) over INTER1V2D (utils/averages.f90:214-239),
 *   local part: inter(j, ip) = count(gate(:, j, :) == ip) / real(nx*nz) for every plane j and level ip = 1 .. np, inter(ny, np) in Fortran
 *   order, HOST memory.  Values of the gate outside 1 .. np, 0 included, are not counted.  On the device all planes and levels come from ONE pass
 *   over the gate (k_gate_count: 32-bit counters in LDS, a second kernel sums the chunks into 64-bit counts and divides once per output); a count
 *   is exact and so is the reference's sum of 1.0, so the result is the reference's bit for bit.  The call synchronises the stream.
 *   TLAB_EINVAL: nx, ny or nz < 1, np outside 1 .. 127, a null pointer. */
int tlab_inter_n_xz(int nx, int ny, int nz, int np, const signed char *gate, double *inter);

/* ---- spectra and correlations in horizontal planes: tools/statistics/spectra.f90 with module SpectraMod (spectra_pool.f90), opt_main 1-4 -------
 * Power and co-spectra E(kx), E(kz), E(kr), E(kx, kz) and auto- and cross-correlations C(rx), C(rz), C(r), C(rx, rz) of a pair of fields per block
 * of nblock y-planes (the uppermost ny mod nblock planes are dropped).  A transformed field is complex (nx/2+1, ny, nz), kx fastest, in the NATURAL
 * kz order of tlab_poisson_fft_x + tlab_poisson_fft_z; the reference's kz shuffle (fft_reordering_k, opr_fourier.f90:357-370) is an index map here,
 * and every 2-D output keeps the reference's shuffled order.  Arrays of a call are all device memory (kernels of csrc/spectra.hip: no atomics, the
 * same bits on every run) or all host memory (the reference's loops, in their order); a mix: TLAB_EINVAL.  Profiles -- variance, var1, var2,
 * variance2, cov, mean: ny doubles per column -- are HOST memory, as in the plane statistics above; a call that returns one synchronises the stream.
 * outx, outz, outr and out2d are ACCUMULATED into (+=, as the reference: a caller can average over times); out2d may be NULL.
 * TLAB_EINVAL: odd nx, nblock < 1 or > ny, kr_total < 1, a null pointer.  TLAB_EUNSUPPORTED: nz = 1, a slab or pencil plan.  Not built: the phase
 * half of REDUCE_SPECTRUM's out, 3-D spectra, masks, MPI.
 * tlab_spectrum_reduce: what spectra.f90:641-650 does to the product of OPR_Fourier_CONVOLUTION_FXZ, from a_hat and b_hat (NULL: an auto pair) in
 *   one read: P = Re(b_hat conj(a_hat)), (P*norm)*norm with norm = 1/(nx*nz); REDUCE_SPECTRUM (:232-274) and INTEGRATE_SPECTRUM (:73-185) into
 *   outx (nx/2, ny/nblock), outz (nz/2, ny/nblock), outr (kr_total, ny/nblock), out2d (nx/2, ny/nblock, nz); variance (ny) is the Parseval control
 *   of REDUCE_SPECTRUM, Nyquist column included, 0 for the dropped planes.
 * tlab_correlation_reduce: spectra.f90:653 and REDUCE_CORRELATION (:313-358) on the real field in (nx, ny, nz) the inverse transforms return:
 *   ((in*norm)*norm) / (sqrt(var1(j)) sqrt(var2(j))) (1 where that product is not positive) summed over the block into outx (nx, ny/nblock; the row
 *   rz = 0), outz (nz, ny/nblock; the column rx = 0), out2d (nx, ny/nblock, nz) and, with icalc_radial = 1, outr (nr_total, ny/nblock);
 *   variance2(j) = (in(1, j, 1)*norm)*norm.
 * tlab_radial_samplesize: RADIAL_SAMPLESIZE (:381-398) counted from zero.  Host arithmetic.
 * tlab_cross_product: c = b_hat conj(a_hat) for n complex numbers (|a_hat|^2 with b_hat NULL); c may be a_hat or b_hat.  Enqueued on the stream.
 * tlab_fluctuation: out = in - mean(j), FI_FLUCTUATION_INPLACE (mappings/fi_dissipation.f90:119-139) into another array with the means of
 *   tlab_avg_ik_v handed in.
 * tlab_avg_cov2v: the three COV2V2D of spectra.f90:624-628 in one pass: cov + (0, 1, 2)*ldcov = plane means of a*b, a*a, b*b (arrays classified
 *   like tlab_avg_ik_v).
 * tlab_spectra_pair: the loop body of spectra.f90:620-659 for one pair of FLUCTUATION fields a, b (NULL or a: auto) on the transforms of a
 *   single-device plan; device arrays only.  mode 1: spectra, 2: correlations (the product, the two inverse transforms, tlab_correlation_reduce with
 *   nr_total = kr_total and the radial sums always taken).  tmp1-3: (nx+2)*ny*nz doubles each, overwritten; a and b are not.  cov (ny, 3): the
 *   covariances a*b, a*a, b*b; variance (ny): variance of mode 1, variance2 of mode 2 -- the reference compares either with cov(:, 1).
 * tlab_dns_spectra: the pairs of spectra.f90:482-522 on the driver's arrays: the variables are u, v, w, (p,) and the nscal scalars; cross = 0: every
 *   variable with itself, cross = 1: uv, uw, vw and us, vs, ws per scalar.  The means are removed into txc[0], txc[1]; txc[3..5] are the work
 *   arrays; q, s, p and the driver state are not touched.  p (NULL: none) must not be one of those five.  Outputs hold one block per pair, back to
 *   back in pair order, each as tlab_spectra_pair writes it. */
int tlab_spectrum_reduce(int nx, int ny, int nz, int nblock, int kr_total, const double *a_hat, const double *b_hat, double *out2d, double *outx,
                         double *outz, double *outr, double *variance);
int tlab_correlation_reduce(int nx, int ny, int nz, int nblock, int nr_total, const double *in, const double *var1, const double *var2, double *out2d,
                            double *outx, double *outz, double *outr, double *variance2, int icalc_radial);
int tlab_radial_samplesize(int nx, int nz, int nr_total, double *samplesize);
int tlab_cross_product(long long n, const double *a_hat, const double *b_hat, double *c);
int tlab_fluctuation(int nx, int ny, int nz, const double *in, const double *mean, double *out);
int tlab_avg_cov2v(int nx, int ny, int nz, const double *a, const double *b, double *cov, int ldcov);
int tlab_spectra_pair(tlab_poisson_plan_t plan, int mode, int nblock, int kr_total, const double *a, const double *b, double *tmp1, double *tmp2,
                      double *tmp3, double *out2d, double *outx, double *outz, double *outr, double *cov, double *variance);
int tlab_dns_spectra(tlab_dns_t h, int mode, int cross, int nblock, int kr_total, double *const *q, double *const *s, double *const *txc,
                     const double *p, double *out2d, double *outx, double *outz, double *outr, double *cov, double *variance);
int tlab_pdf1v_n(int nx, int ny, int nz, int nv, int nbins, const int *ibc, const double *umin, const double *umax, const double *const *u,
                 int igate, const signed char *gate, double *pdf);
int tlab_pdf_minmax_planes(int nx, int ny, int nz, int nv, const double *const *u, int igate, const signed char *gate, double *umin, double *umax);
int tlab_pdf_histogram_planes(int nx, int ny, int nz, int nv, int nbins, const int *ilim, const double *umin, const double *umax,
                              const double *const *u, int igate, const signed char *gate, double *pdf);
int tlab_pdf_analize(int ibc, int nbins, const double *pdf, double *umin, double *umax, double plim, int *nplim);
int tlab_pdf2v(int nx, int ny, int nz, const int *nbins, const double *u, const double *v, double *pdf);
int tlab_gate_threshold(const double *a, long long n, double thr, signed char *gate);
/* The conditional statistics that continue this block -- the partition of FI_GATE, AVG_N_XZ with a gate, RAW_TO_CENTRAL, CAVG1V_N and CAVG2V:
 * tlab_gate_levels, tlab_gate_flux, tlab_dns_gate, tlab_avg_n_xz, tlab_raw_to_central, tlab_cavg1v_n, tlab_cavg2v -- are entry points of the same
 * library, declared with their contract in tlab_amd/csrc/tlab_amd_conditional.h, which includes this header. */

/* RHS_GLOBAL_INCOMPRESSIBLE_1()  tools/dns/rhs_global_incompressible_1.f90:15-405 (argument-less in the reference:
 * it works on the module arrays q, s, hq, hs, txc and on dte).  q[3] = u,v,w; s[nscal]; hq[3], hs[nscal] are
 * accumulated into; txc[9] = tmp1..tmp9, each of isize_txc_field = (nx+2)*ny*nz doubles.  HOST arrays of DEVICE pointers.
 * Convective form, RhsMode = combined.  The flow blocks of the relaxation buffer zones at Jmin / Jmax are applied in the reference's place and the
 * scalars are not relaxed here, as in the reference's RHS; zones at Imin / Imax and filter zones are refused where they are set.  No IBM terms. */
int tlab_rhs_global_incompressible_1(tlab_dns_t d, double dte, double *const *q, double *const *s, double *const *hq,
                                     double *const *hs, double *const *txc);

/* One explicit low-storage Runge-Kutta substep = the unit of the metric:
 * TIME_SUBSTEP_INCOMPRESSIBLE_EXPLICIT (tools/dns/time.f90:559-664): RHS, then q += dte*hq, s += dte*hs;
 * followed, if scale_tendencies != 0, by hq *= kco, hs *= kco (time.f90:261-298, skipped after the last substep). */
int tlab_time_substep_incompressible_explicit(tlab_dns_t d, double dte, double kco, int scale_tendencies,
                                              double *const *q, double *const *s, double *const *hq, double *const *hs,
                                              double *const *txc);

/* ---- the decomposed substep: RHS_GLOBAL_INCOMPRESSIBLE_1 / TIME_SUBSTEP_INCOMPRESSIBLE_EXPLICIT with ims_npro_k > 1 ----------------
 * z-slabs (ims_npro_i x ims_npro_k = 1 x P, base/tlab_mpi_procs.f90:76-94): x- and y-operators are local.  What the reference does with a
 * K-transposition around every z-operator and z-FFT (operators/opr_partial.f90:185-195, 248-253; physics/opr_burgers.f90:386-426;
 * operators/opr_fourier.f90:343-428; base/tlab_mpi_transpose.f90:343-553) is done here without transposing a field for a derivative: the compact
 * z-systems are partitioned at the slab boundaries (tlab_zslab_* above: 3 halo planes of the operand + one value per line and system from each ring
 * neighbour), and the Poisson solver goes z-slab -> kx-pencil with ONE all-to-all after the x-FFT and one per output field on the way back, pipelined
 * in two kx halves against the per-mode solves (tlab_amd/csrc/slab.cpp).  The exchanges go through a transport the caller hands in:
 *   - tlab_comm_slab_transport, in libtlab_amd_comm.so: RCCL grouped ncclSend / ncclRecv on the library's communication stream, so that the x / y
 *     operators on the compute stream (tlab_set_stream) run while halo planes, interface values and pencil blocks travel over xGMI;
 *   - tlab_slab_transport_loopback: all P ranks inside one process on one device (exchanges = device copies): the complete decomposed algorithm
 *     against the single-domain result on a single GPU;
 *   - any other struct of these five entry points: a Fortran host's GPU-aware MPI (MPI_Isend / MPI_Irecv / MPI_Alltoallv on device pointers), or the
 *     host-staged gloo processes of the tests.
 * All counts are doubles, all buffers DEVICE pointers; `stream` is the caller's compute stream (hipStream_t).  An exchange must not start before the
 * work enqueued on `stream` up to the call has finished, and must be complete for the work enqueued on `stream` after `wait` of its ticket. */
typedef struct tlab_slab_transport {
    void *ctx;
    int nranks;           /* ims_npro_k                                                                                              */
    int nlocal;           /* ranks this process executes: 1, or nranks for the single-process loopback                                */
    int first;            /* ims_pro_k of the first (or only) local rank                                                              */
    /* Periodic ring in z.  For the local rank l < nlocal and the message i < nmsg (count[i] doubles): to_left[l*nmsg + i] arrives in from_right[..]
     * of rank - 1, to_right[l*nmsg + i] in from_left[..] of rank + 1.  With two ranks both neighbours are the same peer: sends are posted left then
     * right, receives from the right then from the left.  Returns a ticket >= 0, or a negative TLAB_E* code. */
    int (*ring_start)(void *ctx, void *stream, int nmsg, const long long *count, double *const *to_left, double *const *to_right,
                      double *const *from_right, double *const *from_left);
    /* MPI_Alltoallv among the nranks: send[l] holds the blocks for rank 0, 1, .. back to back, scount[l*nranks + p] doubles each; recv[l] / rcount
     * likewise by source.  Returns a ticket. */
    int (*alltoallv_start)(void *ctx, void *stream, double *const *send, const long long *scount, double *const *recv, const long long *rcount);
    int (*wait)(void *ctx, void *stream, int ticket);
    /* MPI_ALLREDUCE of n HOST doubles per local rank (values[l*n + i]), in place; op 0 = MPI_MAX, 1 = MPI_MIN (tools/dns/time.f90:522),
     * 2 = MPI_SUM (the plane average of the dynamic surface model, boundary_bcs.f90:520) */
    int (*allreduce)(void *ctx, double *values, int n, int op);
    void (*destroy)(void *ctx);     /* may be NULL */
} tlab_slab_transport;
int tlab_slab_transport_loopback(tlab_slab_transport *out, int nranks);

/* ---- x/z pencils: ims_npro_i x ims_npro_k blocks (base/tlab_mpi_procs.f90:76-94), the reference's own scheme ---------------------------------
 * Every x operator through an I-transposition inside ims_comm_x (operators/opr_partial.f90:66-147, physics/opr_burgers.f90:216-262), every z operator
 * through a K-transposition inside ims_comm_z (opr_partial.f90:185-253, opr_burgers.f90:386-426), the operator sequence of
 * tools/dns/rhs_global_incompressible_1.f90:98-398 with its transposed-velocity reuse, the Poisson solver on kx-pencils over all ranks.
 * Exchanges = MPI_Alltoallv inside one of three communicators, supplied by the caller like tlab_slab_transport:
 *   which = 0: all ranks (world order); 1: ims_comm_x of the local rank (members by ims_pro_i); 2: ims_comm_z (members by ims_pro_k).
 *   send[l] holds the blocks for the members back to back, scount[l*size + j] doubles each; recv[l] / rcount likewise by source.
 * Implementations: tlab_pencil_transport_loopback (all ranks in this process, exchanges = device copies), tlab_comm_pencil_transport
 * (libtlab_amd_comm.so: grouped ncclSend / ncclRecv inside the RCCL communicators of tlab_comm_init), or the host's GPU-aware MPI. */
typedef struct tlab_pencil_transport {
    void *ctx;
    int npro_i, npro_k;   /* ims_npro_i, ims_npro_k                                                 */
    int nlocal, first;    /* world ranks this process executes: [first, first + nlocal)             */
    int (*alltoallv_start)(void *ctx, void *stream, int which, double *const *send, const long long *scount, double *const *recv,
                           const long long *rcount);                                                /* returns a ticket >= 0 or a TLAB_E* code */
    int (*wait)(void *ctx, void *stream, int ticket);
    int (*allreduce)(void *ctx, double *values, int n, int op);                                     /* as tlab_slab_transport                  */
    void (*destroy)(void *ctx);                                                                     /* may be NULL                             */
} tlab_pencil_transport;
int tlab_pencil_transport_loopback(tlab_pencil_transport *out, int npro_i, int npro_k);

typedef struct tlab_pencil_dns *tlab_pencil_dns_t;
/* gx, gz: the plans of the GLOBAL x and z directions (nx, nz_total nodes), gy the y plan.  Conditions of the reference's decomposition: nx, nz
 * divisible by npro_i, npro_k; imax even; npro_i divides kmax; imax*jmax divisible by npro_k; at least one kx mode per rank.  The transport context
 * passes to the driver on success only.  Same supported subset as tlab_slab_dns_create (anelastic / dealiasing refused); the driver ADDS to the
 * tendencies like the reference: call tlab_pencil_dns_begin_step (hq = hs = 0) at the start of every Runge-Kutta step. */
int tlab_pencil_dns_create(tlab_pencil_dns_t *out, const tlab_pencil_transport *transport, tlab_fdm_plan_t gx, tlab_fdm_plan_t gy, tlab_fdm_plan_t gz,
                           int nx, int ny, int nz_total, int nscal, double visc, const double *schmidt);
int tlab_pencil_dns_destroy(tlab_pencil_dns_t d);
/* q[3], s[nscal], hq[3], hs[nscal] of imax*jmax*kmax doubles, txc[9] of tlab_pencil_dns_info(d, 3) doubles each, for local rank l */
int tlab_pencil_dns_bind(tlab_pencil_dns_t d, int l, double *const *q, double *const *s, double *const *hq, double *const *hs, double *const *txc);
long long tlab_pencil_dns_info(tlab_pencil_dns_t d, int what);   /* 0 imax, 1 kmax, 2 kmax / npro_i, 3 doubles of a txc array, 4 nlocal, 5 first local rank */
int tlab_pencil_dns_set_bcs(tlab_pencil_dns_t d, const int *flow_jmin, const int *flow_jmax, const int *scal_jmin, const int *scal_jmax);
/* buffer zones, as tlab_dns_set_buffer_zone, for the local rank l with ref for that rank's box (imax, size, kmax, nfields): local, no exchange.
 * tlab_pencil_dns_rhs applies the flow blocks before the pressure forcing, tlab_pencil_dns_substep the scalar blocks before its update. */
int tlab_pencil_dns_set_buffer_zone(tlab_pencil_dns_t d, int l, int end, int group, int size, int nfields, const double *tau, const double *ref);
/* body forces, as tlab_dns_set_coriolis / _set_buoyancy, for every local rank (bbackground is the global profile: every box has the full y extent).
 * tlab_pencil_dns_substep applies them in one launch per rank once the Burgers sums of hq are complete, before the forcing; tlab_pencil_dns_rhs does not. */
int tlab_pencil_dns_set_coriolis(tlab_pencil_dns_t d, int type, const double *vector, const double *parameters);
int tlab_pencil_dns_set_buoyancy(tlab_pencil_dns_t d, int type, const double *vector, int nscalars, const double *parameters, int nparameters,
                                 int inb_scal_array, const double *bbackground);
/* scalar bounds limiting, as tlab_dns_set_scalar_bounds: applied by tlab_pencil_dns_substep in the update pass of each limited scalar */
int tlab_pencil_dns_set_scalar_bounds(tlab_pencil_dns_t d, int n, const int *active, const double *lo, const double *hi);
int tlab_pencil_dns_begin_step(tlab_pencil_dns_t d);
int tlab_pencil_dns_rhs(tlab_pencil_dns_t d, double dte);                                    /* RHS_GLOBAL_INCOMPRESSIBLE_1 */
/* The transpositions are started AHEAD of independent launches (the reference's analogue: tools/dns/rhs_global_incompressible_nbc.f90:135-382): while one
 * operator is applied to a transposed field, the forward transposition of the next field and the backward transposition of the previous result are in
 * flight on the transport's stream; TLAB_PENCIL_OVERLAP=0 (read at creation) keeps the literal sequence.  tlab_pencil_dns_trace: on != 0 records, per
 * RHS, one line per exchange start ("start forward i" / "start backward i"), per launch ("launch operator i" / "launch local") and per wait ("wait
 * forward i" / "wait backward i"); the text of the last RHS is copied into buf (size bytes). */
int tlab_pencil_dns_trace(tlab_pencil_dns_t d, int on, char *buf, int size);
int tlab_pencil_dns_substep(tlab_pencil_dns_t d, double dte, double kco, int scale_tendencies);   /* + the update loops of time.f90:645-664, :272-297 */
/* the monitors, as the slab forms below: TIME_COURANT (pmax, dtime equal on every rank; ds(1) indexed at i + ims_offset_i, ds(3) at k + ims_offset_k),
 * DNS_BOUNDS_CONTROL's DilMin / DilMax and the extremes with their global location (as tlab_dns_dilatation_extremes; all ranks return the same
 * values).  The x / z derivatives go through the I- / K-transpositions where those directions are split; txc[0], txc[1], txc[6], txc[7] are
 * destroyed.  *_courant_local: pmax over the local ranks only, for a host whose own MPI_ALLREDUCE follows (time.f90:522). */
int tlab_pencil_dns_time_courant(tlab_pencil_dns_t d, double cfla, double cfld, double *pmax, double *dtime);
int tlab_pencil_dns_courant_local(tlab_pencil_dns_t d, double *pmax);
int tlab_pencil_dns_dilatation_bounds(tlab_pencil_dns_t d, double *dil_min, double *dil_max);
int tlab_pencil_dns_dilatation_extremes(tlab_pencil_dns_t d, double *dil_min, double *dil_max, int *loc_min, int *loc_max);

typedef struct tlab_slab_dns *tlab_slab_dns_t;
/* gx, gy: the local plans; gz: the plan of the GLOBAL z direction (nz_total nodes).  kmax = nz_total / nranks planes per rank; returns
 * TLAB_EUNSUPPORTED when the slabs are too thin for the partitioned z-systems (kmax <~ 50: tlab_zslab_plan_create) -- such runs keep the
 * reference's K-transposition scheme.  gy_elliptic: NULL, or the y plan of EllipticOrder = CompactDirect6 (tlab_poisson_plan_create_direct).
 * The plans are not owned; the transport struct is copied (its destroy, if any, runs in tlab_slab_dns_destroy).
 * OWNERSHIP of transport->ctx passes to the driver only when the call returns TLAB_OK; on any refusal the caller still owns it and must run
 * transport->destroy(ctx) itself.
 * SUPPORTED SUBSET (everything else is refused with TLAB_EUNSUPPORTED, never silently dropped): convective form, RhsMode = combined, Dirichlet or
 * Neumann walls with an impermeable wall-normal velocity, static or dynamic (linear) scalar surfaces, factorized or CompactDirect6 elliptic solver,
 * remove_divergence on or off; NOT the anelastic formulation or dealiasing filters (single-domain driver tlab_dns_* only). */
int tlab_slab_dns_create(tlab_slab_dns_t *out, const tlab_slab_transport *transport, tlab_fdm_plan_t gx, tlab_fdm_plan_t gy, tlab_fdm_plan_t gz,
                         int nx, int ny, int nz_total, int nscal, double visc, const double *schmidt, tlab_fdm_plan_t gy_elliptic);
int tlab_slab_dns_destroy(tlab_slab_dns_t d);
/* The module arrays of local rank l (0 for a one-rank process): q[3], s[nscal], hq[3], hs[nscal], txc[9] as tlab_rhs_global_incompressible_1
 * (HOST arrays of DEVICE pointers; txc of (nx+2)*ny*kmax doubles each).  Plain arrays: the neighbours' halo planes land in buffers of the driver
 * (the columns of a Fortran host's q(isize_field, 3) lie back to back: there is no room around a field).  The pointers are kept: call again if
 * the host moves its arrays. */
int tlab_slab_dns_bind(tlab_slab_dns_t d, int l, double *const *q, double *const *s, double *const *hq, double *const *hs, double *const *txc);
/* what: 0 kmax, 1 nranks, 2 nlocal, 3 doubles of one halo (3 planes), 4 pipeline stages of the pencil exchange, 5 first local rank,
 * 6 whether the repack passes are folded into the x-transforms (default where the library's own x kernels apply; TLAB_SLAB_FUSED_X=0 at creation
 * keeps the separate passes and rocFFT's inverse, whose results equal the Python driver's to the bit) */
long long tlab_slab_dns_info(tlab_slab_dns_t d, int what);
int tlab_slab_dns_set_bcs(tlab_slab_dns_t d, const int *flow_jmin, const int *flow_jmax, const int *scal_jmin, const int *scal_jmax);
int tlab_slab_dns_begin_step(tlab_slab_dns_t d);                 /* as tlab_dns_begin_step */
/* The deferred tail (tlab_deferred_enable, above) behind the decomposed drivers: the link-time RHS_GLOBAL_INCOMPRESSIBLE_1 of an unpatched host calls these
 * instead of tlab_slab_dns_rhs / tlab_pencil_dns_rhs; the DAXPY / DSCAL calls of time.f90 that follow (tlab_deferred_axpy / _scal on the BOUND arrays of
 * the one local rank) complete the description to tlab_slab_dns_substep / tlab_pencil_dns_substep, zero fills to *_begin_step.  With several local
 * ranks in one process (loopback runs) or the layer off they execute at once. */
int tlab_deferred_slab_rhs(tlab_slab_dns_t d, double dte);
int tlab_deferred_pencil_rhs(tlab_pencil_dns_t d, double dte);
int tlab_slab_dns_set_remove_divergence(tlab_slab_dns_t d, int on);
/* buffer zones, as tlab_dns_set_buffer_zone, for the local rank l (0 .. nlocal-1) with ref for that rank's box (nx, size, kmax, nfields): y is never
 * split, so the relaxation is local and needs no exchange.  The flow blocks act before hq is read for the pressure forcing, the scalar blocks after
 * the wall BCs of hs and before the update (scalars under a zone take a separate update pass). */
int tlab_slab_dns_set_buffer_zone(tlab_slab_dns_t d, int l, int end, int group, int size, int nfields, const double *tau, const double *ref);
/* body forces, as tlab_dns_set_coriolis / _set_buoyancy, for every local rank (bbackground is the global profile: every box has the full y extent).
 * tlab_slab_dns_substep applies them in one launch per rank after the first term of every tendency and before the z pass that finishes the scalars;
 * tlab_slab_dns_rhs does not. */
int tlab_slab_dns_set_coriolis(tlab_slab_dns_t d, int type, const double *vector, const double *parameters);
int tlab_slab_dns_set_buoyancy(tlab_slab_dns_t d, int type, const double *vector, int nscalars, const double *parameters, int nparameters,
                               int inb_scal_array, const double *bbackground);
/* scalar bounds limiting, as tlab_dns_set_scalar_bounds: applied by tlab_slab_dns_substep, one pass per limited scalar after the substep */
int tlab_slab_dns_set_scalar_bounds(tlab_slab_dns_t d, int n, const int *active, const double *lo, const double *hi);
/* as tlab_dns_set_surface_bcs: the dynamic surface model of the scalars on z-slabs.  The plane average of BOUNDARY_BCS_SURFACE_Y (AVG1V2D,
 * boundary_bcs.f90:520,535) is an all-reduce: the transport's allreduce is called with op = 2 (MPI_SUM) on the ranks' plane averages. */
int tlab_slab_dns_set_surface_bcs(tlab_slab_dns_t d, const int *sfc_jmin, const int *sfc_jmax, const double *cpl_jmin, const double *cpl_jmax);      /* as tlab_dns_set_remove_divergence ([Main] TermDivergence) */
/* RHS_GLOBAL_INCOMPRESSIBLE_1 on the bound arrays of all local ranks (tools/dns/rhs_global_incompressible_1.f90:98-398) */
int tlab_slab_dns_rhs(tlab_slab_dns_t d, double dte);
/* TIME_SUBSTEP_INCOMPRESSIBLE_EXPLICIT (tools/dns/time.f90:559-664 + :261-298): RHS with the RK update folded into its last passes */
int tlab_slab_dns_substep(tlab_slab_dns_t d, double dte, double kco, int scale_tendencies);
/* TIME_COURANT with the MPI_MAX of time.f90:522: pmax[2] and dtime (may be NULL) are the same on every rank */
int tlab_slab_dns_time_courant(tlab_slab_dns_t d, double cfla, double cfld, double *pmax, double *dtime);
/* DNS_BOUNDS_CONTROL (tools/dns/dns_local.f90:157-187): extremes of div(q) over the whole box; destroys txc[0], txc[1] */
int tlab_slab_dns_dilatation_bounds(tlab_slab_dns_t d, double *dil_min, double *dil_max);
/* ... and with the global 1-based (i, j, k) of the first occurrence of each (as tlab_dns_dilatation_extremes; loc_* may be NULL): the value is
 * all-reduced first, then the smallest global column-major index among the ranks that hold it.  Destroys txc[0], txc[6], txc[7]. */
int tlab_slab_dns_dilatation_extremes(tlab_slab_dns_t d, double *dil_min, double *dil_max, int *loc_min, int *loc_max);
/* TIME_COURANT's pmax[2] over the local ranks only, for a host whose own MPI_ALLREDUCE follows (time.f90:522) */
int tlab_slab_dns_courant_local(tlab_slab_dns_t d, double *pmax);

/* The pointwise loops of the RHS / RK update as separate calls (rhs_global_incompressible_1.f90:106-112, :197-201, :257-259,
 * :348-352, :279-280, :373-375; time.f90:645-664 + :272-297), for drivers that interleave communication. */
int tlab_pw_add3(double *h, const double *a, const double *b, const double *c, long long n);             /* h += a + b + c   */
int tlab_pw_axpy3(double *o1, double *o2, double *o3, const double *h1, const double *h2, const double *h3,
                  const double *q1, const double *q2, const double *q3, double s, long long n);          /* o = h + q*s, x3  */
int tlab_pw_sum3(double *a, const double *b, const double *c, long long n);                              /* a = a + b + c    */
int tlab_pw_sub3(double *h1, double *h2, double *h3, const double *a, const double *b, const double *c, long long n); /* h -= .., x3 */
int tlab_pw_rk_update(double *q, double *h, double dte, double kco, int scale, long long n);             /* q += dte h; h *= kco */
int tlab_pw_fill(double *a, double value, long long n);      /* a = value   (hq = 0.0_wp at the start of a Runge-Kutta step, time.f90:212-216) */
int tlab_pw_clip(double *a, double lo, double hi, long long n);         /* a = min(max(a, lo), hi)  (DNS_BOUNDS_LIMIT, dns_local.f90:67-90) */
int tlab_pw_scale(double *a, double alpha, long long n);     /* a = alpha a (hq = kco hq between substeps, time.f90:272-297)                    */
/* fused tail of a substep for one field: h -= g (g may be NULL); wall planes of h = pb / pt (NULL = zeros); q += dte h; h *= kco if scale
 * (rhs_global_incompressible_1.f90:348-352, :373-375; time.f90:645-664, :272-297) */
int tlab_pw_final_update(double *q, double *h, const double *g, const double *pb, const double *pt, double dte, double kco, int scale,
                         int nx, int ny, int nz);
int tlab_pw_get_wall_planes(const double *f, double *hb, double *ht, int nx, int ny, int nz);
int tlab_pw_fill_wall_planes(double *f, double vb, double vt, int nx, int ny, int nz);
int tlab_pw_set_wall_planes(double *f, const double *pb, const double *pt, int nx, int ny, int nz);      /* NULL plane = zeros */

/* ---- sampling between two statistics steps: phase averages, towers, saved planes --------------------------------------------------------------
 * What dns_main.f90 does to q, s and the pressure of a substep between two restart files beside the statistics: AvgPhaseSpace / AvgPhaseStress
 * (statistics/avg_phase.f90), DNS_TOWER_ACCUMULATE (tools/dns/dns_tower.f90) and PLANES_SAVE (tools/dns/planes.f90).  No IO: the files stay with
 * the host.  The state that is just arrays is the caller's (avg_flow, avg_stress, tower_buf, data_i / data_j / data_k), so the entry points are
 * stateless but for the tower plan.  Arrays are classified like tlab_avg_ik_v: all in device memory -> the kernels of csrc/sampling.hip; all in host
 * memory (or no tlab_init) -> a host loop that is the reference's statement; a mix: TLAB_EINVAL.  A recorded substep runs first.  No call
 * synchronises the stream: a device accumulator is complete once the stream is (tlab_sync, or a copy on the same stream).
 *
 * tlab_avg_phase_space: AvgPhaseSpaceExec (:123-202) for index 1, 2 or 4 on nf fields (a HOST array of nf pointers; nx*ny*nz doubles each).  avg holds
 *   nx*ny*(avg_planes + 1)*nf doubles in the reference's layout: plane plane_id (1-based) of field f takes localsum = sum over k in increasing k of
 *   field(:,:,k)/g(3)%size, nz_total = g(3)%size (the local part: a z-decomposed host reduces the planes itself), and the last plane, the running
 *   mean, gains that plane / avg_planes.  Every term is a true fp64 division, one point's sum stays in one thread: bit for bit the reference's sum.
 *   TLAB_EINVAL: avg_planes < 1 or plane_id outside 1..avg_planes (the reference divides by zero or writes out of bounds there); avg is untouched.
 * tlab_avg_phase_flow: AvgPhaseSpace(index 1) and AvgPhaseStress (:204-287) in ONE pass over u, v, w: avg_flow (3 fields) and avg_stress (6) in the
 *   same layout, each product rounded before its division.  Stress ids as the calls give them (:230-235): uu 1, uv 2, uw 3, vv 4, vw 5, ww 6.
 * tlab_avg_phase_plane_id: the arithmetic of :142-143, plane_id = mod((itr - 1) - it_first, it_save) + 1 with Fortran's sign of mod, 1 for it_save = 0;
 *   the value is the result (no error code). */
int tlab_avg_phase_space(int nx, int ny, int nz, int nz_total, int nf, const double *const *fields, int avg_planes, int plane_id, double *avg);
int tlab_avg_phase_flow(int nx, int ny, int nz, int nz_total, const double *u, const double *v, const double *w, int avg_planes, int plane_id,
                        double *avg_flow, double *avg_stress);
int tlab_avg_phase_plane_id(int itr, int it_first, int it_save);
/* The towers: tlab_tower_create is DNS_TOWER_INITIALIZE (:62-203) on one rank -- stride: int[3] ([SaveTowers] Stride), nitera_save the number of
 *   time steps the buffer holds -- and keeps tower_ipos, tower_jpos, tower_kpos, tower_accumulation and tower_mode_check.  TLAB_EINVAL where (n - 1)
 *   is a multiple of a stride > 1 in some direction: the reference counts one tower less than it places and writes past tower_ipos.
 * tlab_tower_sizes: long long[8] = tower_imax, tower_jmax, tower_kmax, tower_isize_acc_field, tower_isize_acc_mean, tower_bufsize,
 *   tower_accumulation, tower_mode_check.  tlab_tower_positions: tower_ipos (dir 1), tower_jpos (2) or tower_kpos (3), 1-based.
 * tlab_tower_accumulate: DNS_TOWER_ACCUMULATE (:207-289) into the caller's tower_buf (tower_bufsize doubles, the reference's layout: u, v, w, p, s,
 *   then the five plane means, then t and it; the host's DNS_TOWER_WRITE works on a copy unchanged).  index 1: fields = u, v, w; 2: the first scalar;
 *   4: the pressure (fields: a HOST array of 3 | 1 pointers), which also stores rtime and itime.  The values are v(tower_ipos(ii), tower_jpos(j),
 *   tower_kpos(kk)), j fastest -- the reference's 1:tower_jmax:tower_jstride conforms for stride_y = 1 only, where the two agree.  The means
 *   (TOWER_AVG_IK_V, :502-546) are the sums of k_plane_partial / k_plane_final on the device, the reference's loop on the host, divided by
 *   real(imax*kmax).  tower_accumulation advances when the indices of a step sum to 7.  TLAB_EINVAL, state and buffer untouched: an index that
 *   takes tower_mode_check past 7, a full buffer (tower_accumulation > nitera_save).
 * tlab_tower_reset: tower_accumulation = 1 (the end of DNS_TOWER_WRITE) and tower_mode_check = 0. */
typedef struct tlab_tower *tlab_tower_t;
int tlab_tower_create(tlab_tower_t *out, int nx, int ny, int nz, const int *stride, int nitera_save);
int tlab_tower_destroy(tlab_tower_t t);
int tlab_tower_sizes(tlab_tower_t t, long long *sizes);
int tlab_tower_positions(tlab_tower_t t, int dir, int *pos);
int tlab_tower_accumulate(tlab_tower_t t, int index, const double *const *fields, int itime, double rtime, double *tower_buf);
int tlab_tower_reset(tlab_tower_t t);
/* tlab_planes_gather: the copies of PLANES_SAVE (:279-342) for one direction in one launch.  dir 1: out = data_i(ny, nvars*n, nz) (transposed, j
 *   fastest), 2: data_j(nx, nvars*n, nz), 3: data_k(nx, ny, nvars*n); slot v*n + m holds plane nodes[m] of field v.  nodes: HOST, 1-based, checked as
 *   PLANES_INITIALIZE checks them (TLAB_EINVAL outside 1..the size in that direction); at most 16 fields and 20 planes (vars(16), MAX_SAVEPLANES).
 *   single != 0: out is float, rounded to nearest (IO_TYPE_SINGLE on write); else double.
 * tlab_fi_gradient: FI_GRADIENT (mappings/fi_gradient.f90:26-48), result = (s,x*s,x + s,y*s,y) + s,z*s,z in the reference's order, the derivatives by
 *   the driver's plans with bcs = 0; tmp: nx*ny*nz doubles of work space.  Device arrays.  No IBM.
 * tlab_log10_small: a = log10(a + small_wp), small_wp = 1e-20 (planes.f90:250, :256), arrays of either kind. */
int tlab_planes_gather(int nx, int ny, int nz, int nvars, const double *const *fields, int dir, int n, const int *nodes, void *out, int single);
int tlab_fi_gradient(tlab_dns_t d, const double *s, double *result, double *tmp);
int tlab_log10_small(long long n, double *a);
/* tlab_dns_arm_pressure_sampling: one-shot, like tlab_dns_begin_step.  The next tlab_rhs_global_incompressible_1 or
 *   tlab_time_substep_incompressible_explicit of d takes its samples between the pressure solve and the pressure gradient
 *   (rhs_global_incompressible_1.f90:292-305): tlab_tower_accumulate(tower, 4, p, itime, rtime, tower_buf) and / or tlab_avg_phase_space of p into
 *   phase_avg (nx*ny*(avg_planes + 1) doubles) at plane_id.  Either target may be NULL (both: nothing is armed); the accumulators are DEVICE memory.
 *   On the staggered grid p is interpolated back through OPR_P0_INT_PV in z then x into tmp4 (tmp4 and tmp5 are free there, :294-297); elsewhere the
 *   pressure tmp1 is sampled (the reference hands the solver's work array tmp4 over).  The arm is cleared when taken, also when
 *   that call fails; tlab_dns_pressure (the route that stops at the pressure) refuses an armed driver with TLAB_EUNSUPPORTED and clears it. */
int tlab_dns_arm_pressure_sampling(tlab_dns_t d, tlab_tower_t tower, double *tower_buf, int itime, double rtime, double *phase_avg, int avg_planes,
                                   int plane_id);

/* TLab_Transpose(a, nra, nca, ma, b, mb)   utils/tlab_transpose.f90:14-82 : b(j,i) = a(i,j), bit-exact */
int tlab_transpose(const double *a, int nra, int nca, double *b);

/* which kernel family the last operator call used: 0 none, 1 generic (any n), 2 wave-per-line (x),
 * 3 register-tile (y/z).  For tests / profiling. */
int tlab_last_kernel_path(void);
/* force a kernel family (0 = automatic). */
int tlab_force_kernel_path(int path);
/* tuning knobs for experiments and tests: key 1 = rows per wave of the register-tile kernel (16 | 32 | 64, 0 = automatic); 2 = policy of the half-wave
 * tile kernel (1 off, 2 forced, 0 automatic); 3 = lines per tile of the fused Burgers tiles (16 | 32); 4 = number of persistent workgroups of k_ptile
 * (0 = one per CU, rounded down to a multiple of 8; tests force counts that are not).  Environment switches read once per process (A/B runs):
 * TLAB_XLINE_OCC (1 = the one-wave-per-SIMD form of the fused x-Burgers kernel at 512 points), TLAB_PENCIL_OVERLAP (0 = literal operator sequence of the
 * pencil driver), TLAB_PENTA_TILE_X (0 = pentadiagonal x derivative through two transposes); the others are listed where they are read (csrc/). */
int tlab_set_tuning(int key, int value);

/* Live kernel timing (HIP events on the library's stream around every kernel launch) for bench.py's roofline object.
 * tlab_profile_report writes one line per kernel: "name<TAB>calls<TAB>total_ms<TAB>total_algorithmic_bytes". */
int tlab_profile_enable(int on);
/* tag != NULL and not empty: only launches with exactly this name are timed (two event records per timed launch cost the stream ~3 us each: with
 * every launch of the 512^3 substep timed, 0.2 ms of its 16); NULL or "": all of them. */
int tlab_profile_filter(const char *tag);
int tlab_profile_reset(void);
int tlab_profile_report(char *buf, int nbuf);

/* Debug aid, never on an operator path: runs the *device algorithm's* precomputed tables (chunked Thomas +
 * separator system) through a scalar host emulation so the tables can be checked without a GPU.
 * which = 1 (first derivative, variant ibc) or 2 (second derivative); chunks = number of chunks;
 * f (HOST, n doubles): right-hand side in, solution out. */
int tlab_debug_host_chunked_solve(tlab_fdm_plan_t p, int which, int ibc, int chunks, double *f);
/* Debug aid, never on an operator path: the HOST-factorized tables of the 3- / 7-diagonal first-order integral operators (FDM_Int1_Initialize for
 * SpaceOrder1 = CompactJacobian4 | CompactDirect4 | CompactJacobian6Penta, tlab_amd/csrc/int1_generic.cpp) of the y plan gy for the nm constants
 * lam (ibc: 1 BCS_MIN, 2 BCS_MAX; the sign convention is the caller's), so that they can be checked against the oracle without a GPU.  HOST buffers:
 * fac [nd][n][nm] (nd = RHS diagonals of the derivative), rb, rt [40][nm] (rhs_b(1:5, 0:7), rhs_t(0:4, 1:8)), R [n][LHS diagonals] row-major. */
int tlab_debug_int1_tables(tlab_fdm_plan_t gy, int ibc, int nm, const double *lam, double *fac, double *rb, double *rt, double *R);
/* ... and one FDM_Int1_Solve with them on the DEVICE (k_int1g), two lines per mode.  HOST buffers: f, res [2][n][nm] (res: the solution, boundary
 * values included), bv [2][nm] (the value given at the bottom, ibc = 1, or at the top, 2; the opposite end takes f's entry), du [2][nm].
 * variant (the kernel instantiations the plan builders use): 0 as described; 1: unit forcing (line 0: f = delta at the row opposite to the given
 * end, value 0; line 1: f = 0, value 1; f and bv ignored); 2: ibc = 2 with three lines (f's two and a zero one; values 0, 0, 1), res / du = lines 1, 2. */
/* Debug aid: the pack-layout map tlab_poisson_fft_x_packed works with (host arithmetic, no GPU): element (line, kx) of the complex slab sits at
 * off[kx] + line * width[kx] complex values of the pack buffer -- the layout tlab_pencil_repack_blocks writes for the same nblocks / start / base. */
int tlab_debug_pack_map(int nxh, int nblocks, const int *start, const long long *base, long long *off, int *width);
int tlab_debug_int1_solve(tlab_fdm_plan_t gy, int ibc, int variant, int nm, const double *lam, const double *f, const double *bv, double *res, double *du);

#ifdef __cplusplus
}
#endif
#endif /* TLAB_AMD_H */

/* C ABI of the field mappings of libtlab_amd.so: the reference's mappings/ routines that build the variables of tools/statistics/averages.f90
 * and pdfs.f90 (opt_main 5-8 and after), tools/plot/visuals.f90 and the superlayer tools (csrc/mappings.cpp, kernels in csrc/mappings.hip).  The
 * types, the TLAB_* codes and the conventions are those of include/tlab_amd.h, which this header includes.  It lies beside its sources for the
 * reason tlab_amd_conditional.h does: include/ and the tables of the entry points of include/tlab_amd.h are closed lists that existing tests hold;
 * what those tests ask of a symbol of include/tlab_amd.h, tests/test_mappings_symbols.py asks of the symbols declared here, with
 * tests/mappings_entry_points.py as their table. */
#ifndef TLAB_AMD_MAPPINGS_H
#define TLAB_AMD_MAPPINGS_H

#include "../../include/tlab_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The maps of tlab_gradient_maps: pointwise functions of the nine velocity gradients (and of the scalar gradient where marked s), with their
 * outputs in this order.  Operation order, reference lines:
 *   P                     1  -((u,x + v,y) + w,z)                                             fi_vectorcalculus.f90:129-135
 *   Q                     1                                                                     :199-220
 *   R                     1                                                                     :244-267
 *   STRAIN                1                                                                     fi_strain.f90:76-96
 *   STRAIN_TENSOR         6  Sxx Syy Szz Sxy Sxz Syz                                            :41-58
 *   CURL                  4  wx wy wz, then wx*wx + wy*wy + wz*wz                               fi_vectorcalculus.f90:35-49
 *   VORTICITY             1  the pass of tlab_vorticity_from_gradients                          fi_vorticity.f90:39-51
 *   VORTICITY_PRODUCTION  1                                                                     :75-113
 *   STRAIN_PRODUCTION     1  0.25 x the vorticity production first                              fi_strain.f90:124-160
 *   GRADIENT           s  1                                                                     fi_gradient.f90:26-48
 *   GRADIENT_PRODUCTION s 1                                                                     :63-91
 *   STRAIN_A           s  3  strain1, strain2 (strain1 / G.G where G.G > 0, else strain1), G.G  fi_strain.f90:321-359 */
#define TLAB_MAP_P 0
#define TLAB_MAP_Q 1
#define TLAB_MAP_R 2
#define TLAB_MAP_STRAIN 3
#define TLAB_MAP_STRAIN_TENSOR 4
#define TLAB_MAP_CURL 5
#define TLAB_MAP_VORTICITY 6
#define TLAB_MAP_VORTICITY_PRODUCTION 7
#define TLAB_MAP_STRAIN_PRODUCTION 8
#define TLAB_MAP_GRADIENT 9
#define TLAB_MAP_GRADIENT_PRODUCTION 10
#define TLAB_MAP_STRAIN_A 11
#define TLAB_MAP_COUNT 12
/* The terms of tlab_dns_fi_diffusion */
#define TLAB_FI_VORTICITY_DIFFUSION 0 /* w_i lap w_i            fi_vorticity.f90:133-164 */
#define TLAB_FI_STRAIN_DIFFUSION 1    /* s_ij lap s_ij          fi_strain.f90:180-246    */
#define TLAB_FI_GRADIENT_DIFFUSION 2  /* G_i lap G_i, f = s     fi_gradient.f90:109-130  */
#define TLAB_FI_STRAIN_PRESSURE 3     /* -s_ij p,ij, f = p      fi_strain.f90:264-301    */

/* tlab_gradient_maps: the maps maps[0 .. nmaps-1] (distinct TLAB_MAP_* codes, in any order) of n points in ONE pass (k_gradient_maps): every
 *   gradient a requested map needs is read once, one that none needs is not read; every output is written once.  du9: HOST array of the nine
 *   pointers u,x u,y u,z v,x v,y v,z w,x w,y w,z; ds3: HOST array of s,x s,y s,z, NULL unless a map marked s is requested; out: HOST array of the
 *   output pointers, the outputs of maps[0] first, then those of maps[1], ...  An entry of du9 / ds3 that no requested map needs may be NULL.  No
 *   driver handle.  The arrays read and written are classified like those of tlab_vorticity_from_gradients: all device memory -> the kernel (the
 *   call returns with it enqueued on the library's stream), all host memory or no tlab_init -> a host loop; a mix: TLAB_EINVAL.  Both keep every
 *   operation as the reference writes it -- left-to-right products, no fused multiply-add, IEEE divisions -- so each output equals the statement-
 *   by-statement restatement in every bit, and the bits of a map do not depend on the maps that ride along.  TLAB_EINVAL also: n outside
 *   1 .. 2^31 - 1; nmaps < 1, a code out of range or named twice; a needed pointer NULL; an output that overlaps a given input or another output.
 * tlab_dns_velocity_gradients: OPR_Partial_X/Y/Z(OPR_P1) of q[0..2] by the driver's plans with bcs = 0 into txc9 in the order above.
 * tlab_dns_scalar_gradient: the same of one scalar into ds3.
 * tlab_dns_fi_maps: the two calls above (the second when a map marked s is requested; s and ds3 may be NULL otherwise), then the pass.  The
 *   gradients stay in txc9 / ds3 on return.  This is how FI_STRAIN, FI_STRAIN_TENSOR, FI_INVARIANT_Q, FI_INVARIANT_R, FI_CURL,
 *   FI_VORTICITY_PRODUCTION, FI_STRAIN_PRODUCTION, FI_GRADIENT_PRODUCTION and FI_STRAIN_A run on the device, any set of them from nine (twelve)
 *   derivatives.  The outputs have the reference's operations on the device's derivatives.
 * tlab_dns_fi_diffusion: the term `kind` into result, with the reference's calls in the reference's order: OPR_P1 and OPR_P2 through
 *   tlab_opr_partial (bcs = 0, work6[4] the work array of OPR_P2), combined by k_acc_prod3 / k_acc_prod2 in the reference's operation order.
 *   work6: HOST array of six DEVICE work arrays -- [0] the reference's vort / strain / grad, [1..4] its tmp1 .. tmp4, [5] is not touched.  f: the
 *   scalar (GRADIENT_DIFFUSION) or the pressure (STRAIN_PRESSURE), NULL otherwise; q may be NULL for GRADIENT_DIFFUSION.  No viscosity or
 *   diffusivity is multiplied, as in the reference.
 * The tlab_dns_* entry points take DEVICE arrays (q, txc9, ds3, out, work6: HOST arrays of DEVICE pointers) of nx*ny*nz doubles and refuse with
 *   TLAB_EUNSUPPORTED a driver on the staggered pressure grid and one that holds a z-slab of a larger box (tlab_dns_set_slab); the slab and pencil
 *   drivers have no such entry points.  The library has no immersed boundaries: the reference's IBM branches (ibm_partial, IBM_BCS_FIELD) are not
 *   built.  A pending recorded substep runs before every one of the five.
 * Not built: FI_DISSIPATION, FI_VORTICITY_BAROCLINIC (and so the Baroclinic entry of the enstrophy budget), FI_SOLENOIDAL,
 *   FI_ISOSURFACE_ANGLE / _CURVATURE, TENSOR_EIGENVALUES / TENSOR_EIGENFRAME, and the angles of opt_main = 9. */
int tlab_gradient_maps(long long n, const double *const *du9, const double *const *ds3, const int *maps, int nmaps, double *const *out);
int tlab_dns_velocity_gradients(tlab_dns_t d, double *const *q, double *const *txc9);
int tlab_dns_scalar_gradient(tlab_dns_t d, const double *s, double *const *ds3);
int tlab_dns_fi_maps(tlab_dns_t d, double *const *q, const double *s, const int *maps, int nmaps, double *const *txc9, double *const *ds3,
                     double *const *out);
int tlab_dns_fi_diffusion(tlab_dns_t d, int kind, double *const *q, const double *f, double *result, double *const *work6);

#ifdef __cplusplus
}
#endif

#endif
